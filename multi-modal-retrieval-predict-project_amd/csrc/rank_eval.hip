// Full-ranking label evaluation (compute_ranking_metrics, src/Evaluate/retrieval_overlap.py:84-115; the
// test -> test ground truth's self-exclusion, contructGT.py:73): for every query the first gallery row, in the
// search's order (exact cosine desc, global index asc), that shares a label with it, the number of such rows,
// and the number of rows ranked ahead of a given (score, index) — over the WHOLE gallery, on device.
//
// One contraction, two epilogues.  re_scan: S = Q G^T in f64 on v_mfma_f64_16x16x4_f64 (the library's only
// f64-matrix kernel).  Workgroup = 4 waves = 32 queries x 256 gallery rows, a wave 32 x 64 = 2 x 4 accumulator
// tiles (64 VGPRs); A = queries, B = gallery rows, so a lane (r = lane & 15, h = lane >> 4) holds D[query
// h + 4 reg][row r] of each tile.  Operands go from L2 straight to registers as f32 (queries: the zero-padded
// copy re_prep_queries leaves in the workspace; MMR_F32 gallery rows) or fp16 (MMR_F16: one 16-B tile32h
// piece per lane) and are converted to f64 there, both exactly.  A lane takes k = 32 p + 8 h .. + 7 of step p
// and feeds eight consecutive MFMAs, MFMA j summing k = 32 p + 8 h' + j over h' = 0 .. 3: a k-permutation A
// and B share.  That order is the same for every (query, row) pair, both index dtypes and both epilogues (ONE
// kernel, the epilogue a uniform branch), so byte-identical rows score bit-identically and count_ahead
// reproduces best_relevant's score of a row bit for bit.  Each wave-instruction pair of loads feeds 64 MFMAs
// of 64 cycles: the kernel is MFMA-bound by two orders of magnitude, hence no LDS staging.
//   score = (qn > 0 && gn > 0) ? acc / (qn * gn) : 0.0 (knn.hip's re-score expression; gn = the index's
//   norm64, qn from re_prep_queries in knn_prep_queries' summation order).
//   epilogue 0 (best_relevant): rows < n, != exclude[q], sharing a label bit: the best under (score desc,
//     global index asc) and their count — in-lane over the 4 row tiles, xor 1 / 2 / 4 / 8 over the 16 lanes
//     of a query, the 4 waves through LDS; one (score, index, count) partial per (query, 256-row block).
//   epilogue 1 (count_ahead): rows < n, != exclude[q], with score > ref or (== ref and global index < ref's).
// re_finish_*: one wave per query reduces the row-block partials.  (score, index) is a total order and the
// counts are integers, so no result depends on the order of any reduction: no atomics, identical bytes run to
// run.  Pad rows (>= n) are masked by row number: they score 0, which beats a negative cosine.
#include "knn_index.h"

namespace {

using mmr::aligned16;
using mmr::DeviceGuard;
using mmr::f16x8;
using mmr::f32x4;
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int RE_QT = 32;            // queries per workgroup
constexpr int RE_ROWS = 256;         // gallery rows per workgroup (= kRowPad of knn.hip: Np % 256 == 0)
constexpr int64_t RE_CHUNK = 1024;   // queries per pass (bounds the workspace)
constexpr int64_t RE_NONE = INT64_MAX;

// (score desc, index asc); "none" is (-inf, RE_NONE)
__device__ __forceinline__ bool re_better(double s, int64_t i, double s2, int64_t i2) {
  return s > s2 || (s == s2 && i < i2);
}

// One wave per query row: the zero-padded f32 copy [Qp][Dp] + |q| in f64 (rows >= nq: zeros, norm 0).
__global__ __launch_bounds__(256) void re_prep_queries(const float* __restrict__ q, int64_t nq, int d,
                                                       float* __restrict__ qp, int Dp, int64_t Qp,
                                                       double* __restrict__ qnorm) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= Qp) return;
  double ss = 0.0;
  for (int k = lane; k < Dp; k += 64) {
    const float v = (row < nq && k < d) ? q[row * (int64_t)d + k] : 0.0f;
    qp[row * Dp + k] = v;
    ss += (double)v * (double)v;
  }
  ss = mmr::wave_sum(ss);
  if (lane == 0) qnorm[row] = sqrt(ss);
}

template <bool F16>
struct ReOps {
  f32x4 q[2][2];  // query tile t: k = 8 h .. 8 h + 3 | + 4 .. + 7
  f32x4 g[F16 ? 1 : 4][2];
  f16x8 gh[F16 ? 4 : 1];
};

template <bool F16>
__global__ __launch_bounds__(256) void re_scan(const float* __restrict__ qp, const double* __restrict__ qnorm,
                                               int64_t nq, int nqt, const float* __restrict__ gal,
                                               const uint16_t* __restrict__ galh, int Dp,
                                               const double* __restrict__ gnorm, int64_t n, int64_t idx_base,
                                               int mode, const uint64_t* __restrict__ qlab,
                                               const uint64_t* __restrict__ glab, const int64_t* __restrict__ excl,
                                               const int64_t* __restrict__ ref_idx,
                                               const double* __restrict__ ref_score, double* __restrict__ ps,
                                               int64_t* __restrict__ pi, int32_t* __restrict__ pc, int64_t nrb) {
  __shared__ double sm_s[4][RE_QT];
  __shared__ int64_t sm_i[4][RE_QT];
  __shared__ int32_t sm_c[4][RE_QT];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, h = lane >> 4;
  const int64_t rb = blockIdx.x / nqt;
  const int64_t q0 = (int64_t)(blockIdx.x % nqt) * RE_QT;  // query tile fastest: co-resident workgroups share rows
  const int64_t row0 = rb * RE_ROWS + wave * 64;

  if (mode == 1) {  // count_ahead: a tile whose queries all have ref_idx < 0 does no work
    const bool live = tid < RE_QT && q0 + tid < nq && ref_idx[q0 + tid] >= 0;
    if (!__syncthreads_or(live)) {
      if (tid < RE_QT && q0 + tid < nq) pc[(q0 + tid) * nrb + rb] = 0;
      return;
    }
  }

  const float* qa0 = qp + (q0 + r) * Dp + 8 * h;
  const float* qa1 = qa0 + (int64_t)16 * Dp;
  const float* ga = F16 ? nullptr : gal + (row0 + r) * Dp + 8 * h;
  const uint16_t* gha = F16 ? galh + (row0 >> 4) * (int64_t)(Dp >> 5) * 512 + lane * 8 : nullptr;

  auto load = [&](ReOps<F16>& o, int kb) {
    o.q[0][0] = *(const f32x4*)(qa0 + kb);
    o.q[0][1] = *(const f32x4*)(qa0 + kb + 4);
    o.q[1][0] = *(const f32x4*)(qa1 + kb);
    o.q[1][1] = *(const f32x4*)(qa1 + kb + 4);
    if constexpr (F16) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        o.gh[u] = *(const f16x8*)(gha + ((int64_t)u * (Dp >> 5) + (kb >> 5)) * 512);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        o.g[u][0] = *(const f32x4*)(ga + (int64_t)16 * u * Dp + kb);
        o.g[u][1] = *(const f32x4*)(ga + (int64_t)16 * u * Dp + kb + 4);
      }
    }
  };

  f64x4 acc[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[t][u] = (f64x4){0.0, 0.0, 0.0, 0.0};

  auto mac = [&](const ReOps<F16>& o) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double a0 = (double)o.q[0][j >> 2][j & 3], a1 = (double)o.q[1][j >> 2][j & 3];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        double b;
        if constexpr (F16) b = (double)(float)o.gh[u][j];
        else b = (double)o.g[u][j >> 2][j & 3];
        acc[0][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][u], 0, 0, 0);
        acc[1][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][u], 0, 0, 0);
      }
    }
  };

  // Dp % 64 == 0: an even number of 32-k steps, the next one's loads in flight under each step's 64 MFMAs
  ReOps<F16> oa, ob;
  load(oa, 0);
  for (int kb = 0; kb < Dp; kb += 64) {
    load(ob, kb + 32);
    mac(oa);
    if (kb + 64 < Dp) load(oa, kb + 64);
    mac(ob);
  }

  // lane: rows row0 + 16 u + r, queries q0 + 16 t + h + 4 reg
  double gn[4];
  uint64_t gl[4];
  int64_t gi[4];
  bool gok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t row = row0 + 16 * u + r;
    gok[u] = row < n;
    gn[u] = gnorm[row];
    gi[u] = row + idx_base;
    gl[u] = (mode == 0 && gok[u]) ? glab[row] : 0;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int ql_ = 16 * t + h + 4 * reg;
      const int64_t qi = q0 + ql_;
      const bool qok = qi < nq;
      const double qn = qnorm[qi];
      const int64_t ex = (excl && qok) ? excl[qi] : -1;
      double bs = -INFINITY;
      int64_t bi = RE_NONE;
      int32_t cnt = 0;
      if (mode == 0) {
        const uint64_t ql = qok ? qlab[qi] : 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double s = (qn > 0.0 && gn[u] > 0.0) ? acc[t][u][reg] / (qn * gn[u]) : 0.0;
          if (gok[u] && gi[u] != ex && (gl[u] & ql) != 0) {
            ++cnt;
            if (re_better(s, gi[u], bs, bi)) {
              bs = s;
              bi = gi[u];
            }
          }
        }
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
          const double s2 = __shfl_xor(bs, m, 64);
          const int64_t i2 = __shfl_xor((long long)bi, m, 64);
          cnt += __shfl_xor(cnt, m, 64);
          if (re_better(s2, i2, bs, bi)) {
            bs = s2;
            bi = i2;
          }
        }
      } else {
        const int64_t ri = qok ? ref_idx[qi] : -1;
        const double rs = ri >= 0 ? ref_score[qi] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double s = (qn > 0.0 && gn[u] > 0.0) ? acc[t][u][reg] / (qn * gn[u]) : 0.0;
          if (gok[u] && gi[u] != ex && ri >= 0 && re_better(s, gi[u], rs, ri)) ++cnt;
        }
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) cnt += __shfl_xor(cnt, m, 64);
      }
      if (r == 0) {
        sm_s[wave][ql_] = bs;
        sm_i[wave][ql_] = bi;
        sm_c[wave][ql_] = cnt;
      }
    }
  }
  __syncthreads();
  if (tid < RE_QT && q0 + tid < nq) {
    double bs = sm_s[0][tid];
    int64_t bi = sm_i[0][tid];
    int32_t cnt = sm_c[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      cnt += sm_c[w][tid];
      if (re_better(sm_s[w][tid], sm_i[w][tid], bs, bi)) {
        bs = sm_s[w][tid];
        bi = sm_i[w][tid];
      }
    }
    const int64_t o = (q0 + tid) * nrb + rb;
    pc[o] = cnt;
    if (mode == 0) {
      ps[o] = bs;
      pi[o] = bi;
    }
  }
}

// One wave per query: the row-block partials -> the query's result.
__global__ __launch_bounds__(256) void re_finish_best(const double* __restrict__ ps, const int64_t* __restrict__ pi,
                                                      const int32_t* __restrict__ pc, int64_t nrb, int64_t nq,
                                                      int64_t* __restrict__ out_idx, double* __restrict__ out_score,
                                                      int64_t* __restrict__ out_nrel) {
  const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (qi >= nq) return;
  double bs = -INFINITY;
  int64_t bi = RE_NONE, cnt = 0;
  for (int64_t b = lane; b < nrb; b += 64) {
    const int64_t o = qi * nrb + b;
    cnt += pc[o];
    if (re_better(ps[o], pi[o], bs, bi)) {
      bs = ps[o];
      bi = pi[o];
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double s2 = __shfl_xor(bs, m, 64);
    const int64_t i2 = __shfl_xor((long long)bi, m, 64);
    cnt += __shfl_xor((long long)cnt, m, 64);
    if (re_better(s2, i2, bs, bi)) {
      bs = s2;
      bi = i2;
    }
  }
  if (lane == 0) {
    const bool none = bi == RE_NONE;
    out_idx[qi] = none ? -1 : bi;
    if (out_score) out_score[qi] = none ? 0.0 : bs;
    if (out_nrel) out_nrel[qi] = cnt;
  }
}

__global__ __launch_bounds__(256) void re_finish_count(const int32_t* __restrict__ pc, int64_t nrb, int64_t nq,
                                                       int64_t* __restrict__ out_ahead) {
  const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (qi >= nq) return;
  int64_t cnt = 0;
  for (int64_t b = lane; b < nrb; b += 64) cnt += pc[qi * nrb + b];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor((long long)cnt, m, 64);
  if (lane == 0) out_ahead[qi] = cnt;
}

// Workspace of a pass of c (% 32 == 0) queries: [qp f32 c x Dp | qnorm f64 c | ps f64 | pi i64 | pc i32, c x nrb]
struct ReWork {
  float* qp;
  double* qnorm;
  double* ps;
  int64_t* pi;
  int32_t* pc;
  int64_t bytes;
};
inline int64_t re_chunk(int64_t nq) { return nq < RE_CHUNK ? mmr::round_up(nq, RE_QT) : RE_CHUNK; }
inline ReWork re_layout(const mmr_index* ix, int64_t c, void* work) {
  const int64_t nrb = ix->Np / RE_ROWS;
  char* p = (char*)work;
  ReWork w;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* at = p + off;
    off += mmr::round_up(bytes, 256);
    return at;
  };
  w.qp = (float*)take(c * ix->Dp * 4);
  w.qnorm = (double*)take(c * 8);
  w.ps = (double*)take(c * nrb * 8);
  w.pi = (int64_t*)take(c * nrb * 8);
  w.pc = (int32_t*)take(c * nrb * 4);
  w.bytes = off;
  return w;
}

// mode 0: best_relevant, mode 1: count_ahead — queries in passes of <= RE_CHUNK
mmr_status re_run(const mmr_index* ix, const float* q, int64_t nq, int mode, const uint64_t* q_labels,
                  const uint64_t* g_labels, const int64_t* exclude, const int64_t* ref_idx, const double* ref_score,
                  int64_t* out_idx, double* out_score, int64_t* out_cnt, void* work, void* stream) {
  DeviceGuard g(ix->device);
  hipStream_t st = mmr::as_stream(stream);
  const int64_t nrb = ix->Np / RE_ROWS;
  const ReWork w = re_layout(ix, re_chunk(nq), work);
  const bool f16 = ix->dtype == MMR_F16;
  for (int64_t p0 = 0; p0 < nq; p0 += RE_CHUNK) {
    const int64_t c = nq - p0 < RE_CHUNK ? nq - p0 : RE_CHUNK;
    const int64_t cp = mmr::round_up(c, RE_QT);
    const int nqt = (int)(cp / RE_QT);
    re_prep_queries<<<dim3((unsigned)mmr::ceil_div(cp, 4)), 256, 0, st>>>(q + p0 * ix->d, c, ix->d, w.qp, ix->Dp, cp,
                                                                         w.qnorm);
    const dim3 grid((unsigned)(nrb * nqt));
    const uint64_t* ql = q_labels ? q_labels + p0 : nullptr;
    const int64_t* ex = exclude ? exclude + p0 : nullptr;
    const int64_t* ri = ref_idx ? ref_idx + p0 : nullptr;
    const double* rs = ref_score ? ref_score + p0 : nullptr;
    if (f16)
      re_scan<true><<<grid, 256, 0, st>>>(w.qp, w.qnorm, c, nqt, nullptr, ix->gh, ix->Dp, ix->norm64, ix->n, ix->idx_base,
                                          mode, ql, g_labels, ex, ri, rs, w.ps, w.pi, w.pc, nrb);
    else
      re_scan<false><<<grid, 256, 0, st>>>(w.qp, w.qnorm, c, nqt, ix->gal, nullptr, ix->Dp, ix->norm64, ix->n,
                                           ix->idx_base, mode, ql, g_labels, ex, ri, rs, w.ps, w.pi, w.pc, nrb);
    const dim3 fgrid((unsigned)mmr::ceil_div(c, 4));
    if (mode == 0)
      re_finish_best<<<fgrid, 256, 0, st>>>(w.ps, w.pi, w.pc, nrb, c, out_idx + p0, out_score ? out_score + p0 : nullptr,
                                            out_cnt ? out_cnt + p0 : nullptr);
    else
      re_finish_count<<<fgrid, 256, 0, st>>>(w.pc, nrb, c, out_cnt + p0);
    MMR_LAUNCH_CHECK();
  }
  return MMR_OK;
}

}  // namespace

extern "C" {

int64_t mmr_index_rank_work_bytes(const mmr_index* ix, int64_t nq) {
  if (!ix || nq <= 0) return 0;
  return re_layout(ix, re_chunk(nq), nullptr).bytes;
}

mmr_status mmr_index_best_relevant(const mmr_index* ix, const float* q, int64_t nq, const uint64_t* q_labels,
                                   const uint64_t* g_labels, const int64_t* exclude, int64_t* out_idx,
                                   double* out_score, int64_t* out_nrel, void* work, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(ix != nullptr, "mmr_index_best_relevant: index is NULL");
  MMR_REQUIRE(nq >= 0, "mmr_index_best_relevant: nq < 0");
  if (nq == 0) return MMR_OK;
  MMR_REQUIRE(q && q_labels && out_idx, "mmr_index_best_relevant: NULL q / q_labels / out_idx");
  MMR_REQUIRE(ix->n == 0 || g_labels, "mmr_index_best_relevant: g_labels is NULL");
  MMR_REQUIRE(work && aligned16(work), "mmr_index_best_relevant: work is NULL or not 16-B aligned");
  return re_run(ix, q, nq, 0, q_labels, g_labels, exclude, nullptr, nullptr, out_idx, out_score, out_nrel, work, stream);
}

mmr_status mmr_index_count_ahead(const mmr_index* ix, const float* q, int64_t nq, const int64_t* ref_idx,
                                 const double* ref_score, const int64_t* exclude, int64_t* out_ahead, void* work,
                                 void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(ix != nullptr, "mmr_index_count_ahead: index is NULL");
  MMR_REQUIRE(nq >= 0, "mmr_index_count_ahead: nq < 0");
  if (nq == 0) return MMR_OK;
  MMR_REQUIRE(q && ref_idx && ref_score && out_ahead, "mmr_index_count_ahead: NULL q / ref_idx / ref_score / out_ahead");
  MMR_REQUIRE(work && aligned16(work), "mmr_index_count_ahead: work is NULL or not 16-B aligned");
  return re_run(ix, q, nq, 1, nullptr, nullptr, exclude, ref_idx, ref_score, nullptr, nullptr, out_ahead, work, stream);
}

}  // extern "C"
