// Batched DenseLinkSearch walk (DLSRetrievalEngine.retrieve, src/Retrieval/retrieval.py:198-244) on device:
// mmr_index_dls_walk (include/mmr.h holds the semantics, the score expression, the tie rules and the limits).
//
// The walk is sequential per query and bound by latency: a step is the read of the best candidate's neighbour
// row, then the read of the unvisited neighbours' gallery rows, then a few hundred VALU / LDS instructions.  One
// wavefront walks one query (a 64-thread workgroup: no barrier is shared with another query), the query sits in
// registers as f64, the candidate set and the visited set in LDS:
//   candidate set  a list sorted by (score desc, index asc), two buffers of r entries (f64 score, int32 row).
//                  A step pops the head and merges the <= 32 new entries into the other buffer: every kept
//                  entry moves down by the number of new entries ahead of it, every new entry lands behind the
//                  kept entries ahead of it (counted with one ballot per new entry and 64 kept entries) plus its
//                  rank among the new ones; positions >= r are dropped, which is the reference's truncation
//                  (heapq.nsmallest(R)).  (score, index) is a strict total order over distinct rows, so the list
//                  does not depend on which lane carried which neighbour.
//   visited set    open addressing over H >= 2 x (the most rows a walk can visit) int32 slots, one LDS
//                  compare-and-swap per probe: a neighbour is new iff its CAS found the slot empty, which also
//                  settles a row listed twice in one neighbour row.
//   scores         all unvisited neighbours of a step are known after ONE round of probes; their rows are then
//                  loaded in batches of up to DW_RB = 16 rows (8 for d > 768), every load of a batch issued before
//                  its first FMA (<= 48 float4 per lane in flight: more spills), so a step of <= 16 new rows costs
//                  one row latency (the engine's default max_links = 10 never needs a second batch).  The row
//                  norms are requested before the rows.  A lane owns the floats 256 c + 4 lane .. + 3 of every
//                  256-float chunk c and accumulates them in ascending order with f64 FMAs; the 64 partials go
//                  through wave_sum's tree (rows_wave_sum, eight rows per call, bit-identical to wave_sum).  The
//                  shape is the same for every row whatever the batch slot, the batch width, the neighbour
//                  position or the number of rows loaded with it, so byte-identical rows score bit-identically.
// Measured (profiles/dls_walk.txt, 100k x 768, K = 5): ~3.2 us per step, most of it the lone wave's own instruction
// issue; 25.7 us for one query (6 steps), 312 us for 256 (longest walk 97 steps).
#include <type_traits>

#include "knn_index.h"

namespace {

using mmr::DeviceGuard;

constexpr int DW_MAX_R = 512;        // candidate-set bound r
constexpr int DW_MAX_LINKS = 32;     // neighbour-row width (one lane per neighbour, <= 32 new rows per step)
constexpr int DW_MAX_VISIT = 4096;   // rows a walk can visit: min(n, seed_size + max_steps * max_links)
constexpr int DW_MAX_DP = 1024;      // padded row length (d <= 1024)

__device__ __forceinline__ bool dw_better(double s, int i, double s2, int i2) {
  return s > s2 || (s == s2 && i < i2);
}
__device__ __forceinline__ int dw_lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double dw_lane_d(double v, int l) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// LDS of one walk: [cs f64 2 x rc | dots f64 32 | ci i32 2 x rc | fresh i32 32 | tab i32 H], rc = r rounded up
// to even (every region 16-B aligned)
inline size_t dw_lds_bytes(int r, int H) {
  const int rc = (r + 1) & ~1;
  return (size_t)(2 * rc + 32) * 12 + (size_t)H * 4;
}

template <int NC>
__global__ __launch_bounds__(64) void dls_walk_kernel(
    const float* __restrict__ gal, int Dp, const double* __restrict__ gnorm, int64_t n, int64_t idx_base,
    const float* __restrict__ q, int d, const int64_t* __restrict__ nbr, int max_links,
    const int64_t* __restrict__ seeds, int seed_size, int k, int max_steps, int r, int log_h,
    int64_t* __restrict__ out_idx, float* __restrict__ out_score, double* __restrict__ out_score64,
    int32_t* __restrict__ out_steps, int32_t* __restrict__ out_visited) {
  constexpr int DW_RB = NC <= 3 ? 16 : 8;  // rows per load batch: <= 48 float4 per lane in flight
  extern __shared__ __attribute__((aligned(16))) unsigned char dw_smem[];
  const int lane = threadIdx.x;
  const int64_t qi = blockIdx.x;
  const int rc = (r + 1) & ~1;
  double* cs = (double*)dw_smem;
  double* dots = cs + 2 * rc;
  int* ci = (int*)(dots + 32);
  int* fresh = ci + 2 * rc;
  int* tab = fresh + 32;
  const int H = 1 << log_h;
  const uint32_t hmask = (uint32_t)H - 1u;

  for (int i = lane; i < H / 4; i += 64) ((int4*)tab)[i] = make_int4(-1, -1, -1, -1);

  // the query in registers: lane's floats of every chunk, as f64; |q| + 1e-6
  // (every element is loaded from a clamped address and masked after, so the loads are independent of each
  // other; goff[c]: the lane's float offset in a padded gallery row, for a chunk position past the row a valid
  // one whose product meets a zero of the query)
  double qd[NC][4];
  float qf[NC][4];
  int goff[NC];
  double ss = 0.0;
  const float* qrow = q + qi * (int64_t)d;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int k0 = c * 256 + lane * 4;
    goff[c] = k0 < Dp ? k0 : (lane & 15) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) qf[c][e] = qrow[k0 + e < d ? k0 + e : 0];
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double v = c * 256 + lane * 4 + e < d ? (double)qf[c][e] : 0.0;
      qd[c][e] = v;
      ss = fma(v, v, ss);
    }
  }
  const double qn = sqrt(mmr::wave_sum(ss)) + 1e-6;
  __syncthreads();

  int cur = 0, L = 0, head = 0, steps = 0, nvis = 0, seed_pos = 0;
  for (;;) {
    // ---- the rows to absorb: the next <= 32 seeds, or the neighbours of the best candidate (which is popped)
    int64_t v = -1;
    int pop;
    if (seed_pos < seed_size) {
      const int s = seed_pos + lane;
      if (lane < 32 && s < seed_size) v = seeds[qi * (int64_t)seed_size + s];
      seed_pos += 32;
      pop = 0;
    } else {
      if (steps >= max_steps || L == 0) break;
      const int64_t best = __builtin_amdgcn_readfirstlane(ci[cur * rc]);
      if (lane < max_links) v = nbr[best * max_links + lane];
      pop = 1;
    }

    // ---- visited check of all of them, then compaction of the new rows to lanes 0 .. m - 1
    const bool ok = v >= 0 && v < n;
    const int vi = (int)v;
    bool isnew = false;
    if (ok) {
      uint32_t h = ((uint32_t)vi * 2654435761u) >> (32 - log_h);
      for (;;) {
        const int old = atomicCAS(&tab[h], -1, vi);
        if (old == -1) {
          isnew = true;
          break;
        }
        if (old == vi) break;
        h = (h + 1u) & hmask;
      }
    }
    const uint64_t bal = __ballot(isnew);
    const int m = __popcll(bal);
    if (m == 0) {
      if (pop) {  // nothing added: the walk stops, the step is not counted, the popped row is gone
        head = 1;
        break;
      }
      continue;
    }
    if (isnew) fresh[__popcll(bal & ((1ull << lane) - 1ull))] = vi;
    __syncthreads();
    const int ni = lane < m ? fresh[lane] : 0;
    const double gn = lane < m ? gnorm[ni] : 0.0;  // in flight under the row loads
    nvis += m;

    // ---- <row, q> of the new rows, up to DW_RB rows per batch, every load of a batch before its first FMA.  A
    // batch runs at the narrowest width R in {4, 8, 16} that holds it (a lone wave pays every instruction it
    // issues: a 16-row body for the usual 1 - 4 new rows cost more than the loads it waits for); every width
    // reduces a row through the same tree, rows_wave_sum<8> (with its 2- and 4-row forms this kernel compiled to
    // 32 B of scratch per lane)
    auto batch = [&](auto width, int b0, int cnt) {
      constexpr int R = decltype(width)::value;
      float4 g[R][NC];
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        if (rr < cnt) {
          const int row = dw_lane_i(ni, b0 + rr);
          const float* p = gal + (int64_t)row * Dp;
#pragma unroll
          for (int c = 0; c < NC; ++c) g[rr][c] = *(const float4*)(p + goff[c]);
        } else {
#pragma unroll
          for (int c = 0; c < NC; ++c) g[rr][c] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      double a0[8] = {}, a1[8] = {};
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        double acc = 0.0;
        if (rr < cnt) {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            mmr::pin(g[rr][c].x);
            mmr::pin(g[rr][c].y);
            mmr::pin(g[rr][c].z);
            mmr::pin(g[rr][c].w);
            acc = fma((double)g[rr][c].x, qd[c][0], acc);
            acc = fma((double)g[rr][c].y, qd[c][1], acc);
            acc = fma((double)g[rr][c].z, qd[c][2], acc);
            acc = fma((double)g[rr][c].w, qd[c][3], acc);
          }
        }
        if (rr < 8) a0[rr] = acc;
        else a1[rr & 7] = acc;
      }
      int row;
      const double t0 = mmr::rows_wave_sum<8>(a0, lane, row);
      if ((lane & 7) == 0) dots[b0 + row] = t0;  // the lanes that hold each row once
      if constexpr (R > 8) {
        const double t1 = mmr::rows_wave_sum<8>(a1, lane, row);
        if ((lane & 7) == 0) dots[b0 + 8 + row] = t1;
      }
    };
    for (int b0 = 0; b0 < m; b0 += DW_RB) {
      const int cnt = m - b0;
      if (cnt <= 4) batch(std::integral_constant<int, 4>{}, b0, cnt);
      else if (cnt <= 8 || DW_RB == 8) batch(std::integral_constant<int, 8>{}, b0, cnt);
      else batch(std::integral_constant<int, DW_RB>{}, b0, cnt);
    }
    __syncthreads();
    const double ns = lane < m ? dots[lane] / fma(gn, qn, 1e-12) : 0.0;

    // ---- merge into the other buffer (the head dropped when this is a step)
    int nrank = 0;
    for (int t = 0; t < m; ++t) nrank += dw_better(dw_lane_d(ns, t), dw_lane_i(ni, t), ns, ni) ? 1 : 0;
    const double* sA = cs + cur * rc;
    const int* iA = ci + cur * rc;
    double* sB = cs + (cur ^ 1) * rc;
    int* iB = ci + (cur ^ 1) * rc;
    int before = 0;
    for (int p0 = pop; p0 < L; p0 += 64) {
      const int p = p0 + lane;
      const bool act = p < L;
      const double es = act ? sA[p] : 0.0;
      const int ei = act ? iA[p] : 0;
      int shift = 0;
      for (int t = 0; t < m; ++t) {
        const bool nb = dw_better(dw_lane_d(ns, t), dw_lane_i(ni, t), es, ei);
        shift += nb ? 1 : 0;
        const int ahead = __popcll(__ballot(act && !nb));
        if (lane == t) before += ahead;
      }
      const int dest = p - pop + shift;
      if (act && dest < r) {
        sB[dest] = es;
        iB[dest] = ei;
      }
    }
    if (lane < m) {
      const int dest = before + nrank;
      if (dest < r) {
        sB[dest] = ns;
        iB[dest] = ni;
      }
    }
    L = L - pop + m;
    L = L < r ? L : r;
    cur ^= 1;
    __syncthreads();
    steps += pop;
  }

  // ---- the best min(k, |set|) in (score desc, index desc): a run of equal scores is written back to front
  const double* sA = cs + cur * rc + head;
  const int* iA = ci + cur * rc + head;
  const int len = L - head;
  const int kk = k < len ? k : len;
  for (int p = lane; p < k; p += 64) {
    const int64_t o = qi * (int64_t)k;
    if (p < kk) {
      const double s = sA[p];
      int gs = p, ge = p + 1;
      while (gs > 0 && sA[gs - 1] == s) --gs;
      while (ge < kk && sA[ge] == s) ++ge;
      const int pos = gs + (ge - 1 - p);
      out_idx[o + pos] = (int64_t)iA[p] + idx_base;
      out_score[o + pos] = (float)s;
      if (out_score64) out_score64[o + pos] = s;
    } else {
      out_idx[o + p] = -1;
      out_score[o + p] = -INFINITY;
      if (out_score64) out_score64[o + p] = -INFINITY;
    }
  }
  if (lane == 0) {
    if (out_steps) out_steps[qi] = steps;
    if (out_visited) out_visited[qi] = nvis;
  }
}

}  // namespace

extern "C" {

mmr_status mmr_index_dls_walk(const mmr_index* ix, const float* q, int64_t nq, const int64_t* nbr, int32_t max_links,
                              const int64_t* seeds, int32_t seed_size, int32_t k, int32_t max_steps, int32_t r,
                              int64_t* out_idx, float* out_score, double* out_score64, int32_t* out_steps,
                              int32_t* out_visited, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(ix != nullptr, "mmr_index_dls_walk: index is NULL");
  if (ix->dtype != MMR_F32) {
    mmr::set_error("mmr_index_dls_walk: a native fp16 index (MMR_F16) is not supported, the walk reads f32 rows");
    return MMR_ERR_UNSUPPORTED;
  }
  MMR_REQUIRE(nq >= 0 && nq <= INT32_MAX, "mmr_index_dls_walk: nq outside [0, 2^31 - 1]");
  MMR_REQUIRE(r >= 1 && r <= DW_MAX_R, "mmr_index_dls_walk: r=%d outside [1, %d]", r, DW_MAX_R);
  MMR_REQUIRE(max_links >= 1 && max_links <= DW_MAX_LINKS, "mmr_index_dls_walk: max_links=%d outside [1, %d]",
              max_links, DW_MAX_LINKS);
  MMR_REQUIRE(k >= 1 && k <= r, "mmr_index_dls_walk: k=%d outside [1, r=%d]", k, r);
  MMR_REQUIRE(seed_size >= 0 && seed_size <= r, "mmr_index_dls_walk: seed_size=%d outside [0, r=%d]", seed_size, r);
  MMR_REQUIRE(max_steps >= 0, "mmr_index_dls_walk: max_steps=%d < 0", max_steps);
  MMR_REQUIRE(ix->n <= INT32_MAX, "mmr_index_dls_walk: the index has more than 2^31 - 1 rows");
  MMR_REQUIRE(ix->Dp <= DW_MAX_DP, "mmr_index_dls_walk: d=%d exceeds the limit %d", ix->d, DW_MAX_DP);
  int64_t visit = (int64_t)seed_size + (int64_t)max_steps * max_links;
  if (visit > ix->n) visit = ix->n;
  MMR_REQUIRE(visit <= DW_MAX_VISIT,
              "mmr_index_dls_walk: min(n, seed_size + max_steps * max_links) = %lld exceeds the visited-set limit %d",
              (long long)visit, DW_MAX_VISIT);
  if (nq == 0) return MMR_OK;
  MMR_REQUIRE(q && nbr && out_idx && out_score && (seeds || seed_size == 0),
              "mmr_index_dls_walk: NULL q / nbr / seeds / out_idx / out_score");
  int log_h = 8;
  while ((1 << log_h) < 2 * visit) ++log_h;
  const size_t lds = dw_lds_bytes(r, 1 << log_h);
  DeviceGuard g(ix->device);
  hipStream_t st = mmr::as_stream(stream);
  const dim3 grid((unsigned)nq);
  mmr::pick_ceil<1, 2, 3, 4>((int)((ix->Dp + 255) / 256), [&](auto nc) {
    dls_walk_kernel<nc()><<<grid, 64, lds, st>>>(ix->gal, ix->Dp, ix->norm64, ix->n, ix->idx_base, q, ix->d, nbr,
                                                 max_links, seeds, seed_size, k, max_steps, r, log_h, out_idx, out_score,
                                                 out_score64, out_steps, out_visited);
  });
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

}  // extern "C"
