// Map alignment (the reference's compare_maps, src/Helpers/helper.py:173-209, as the explanation evaluation
// src/Evaluate/retrieval_explain_eval.py runs it per query): for P pairs (pa[p], pb[p]) over N maps of HW pixels —
// Pearson, Spearman and the intersection / union counts of the top-k_j pixels, on device.  Every output is an
// integer, an order statistic or an f64 sum in a fixed order: no float atomics, identical bytes run to run.
//
// Per map, once.  ma_build_keys writes one u64 per pixel: [map : bits 48.. | image : bits 16..47 | pixel : bits
// 0..15], image = the order-preserving u32 image of the f32 (-0 canonicalised to +0): all ordering comes from
// integer compares.  One stable LSD radix sort (radix_sort.h, the classifier evaluation's) over the bits
// [16, 48 + ceil(log2 N)) leaves map m the ascending segment [m HW, (m + 1) HW).  ma_ranks gives every key the
// doubled average rank of its tie group, start + end + 1 (start = the group's first position, end = one past its
// last; 2 x scipy rankdata's 'average'), found by a lower / upper bound search in the segment (skipped where the
// neighbour already differs), and scatters it back to pixel order.  ma_map_stats (workgroup per map): the k_j-th
// largest values, the constant flag (first image == last), the f64 mean and sum of (x - mean)^2.
// Per pair, ma_pair (workgroup per pair): Sab = sum (a - mean_a)(b - mean_b) in f64; with the centred doubled ranks
// c = 2 r - (HW + 1) the exact int64 sums S_ab, S_aa, S_bb (|c| <= HW <= 65536: each <= 2.9e14); inter_j / union_j
// of (a >= ta_j), (b >= tb_j).  pearson = Sab / sqrt(ssd_a ssd_b), spearman = S_ab / sqrt(S_aa S_bb) — the root of
// the product, so a self-pair gives exactly 1 (sqrt(fl(x x)) == x); both 0.0 when either map is constant
// (helper.py:188-190).  Pair entries outside [0, N) are flagged and skipped.
#include "common.h"

#pragma clang fp contract(off)

namespace {

using mmr::aligned16;

#include "radix_sort.h"

constexpr int MA_MAXF = 4;

__device__ __forceinline__ uint32_t ma_image(uint32_t u) {  // ascending; -0 -> +0
  if ((u << 1) == 0) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t ma_image_bits(uint32_t asc) {
  return (asc & 0x80000000u) ? (asc ^ 0x80000000u) : ~asc;
}
__device__ __forceinline__ uint32_t ma_key_image(uint64_t k) { return (uint32_t)(k >> 16); }

__global__ __launch_bounds__(256) void ma_build_keys(const uint32_t* __restrict__ maps, int64_t ld, uint32_t hw,
                                                     uint32_t m, uint64_t* __restrict__ keys,
                                                     unsigned long long* __restrict__ nonfinite) {
  const uint32_t stride = gridDim.x * 256u;
  for (uint64_t e64 = (uint64_t)blockIdx.x * 256u + threadIdx.x; e64 < m; e64 += stride) {
    const uint32_t e = (uint32_t)e64;
    const uint32_t map = e / hw, px = e - map * hw;
    const uint32_t u = maps[(int64_t)map * ld + px];
    if ((u & 0x7F800000u) == 0x7F800000u) atomicAdd(nonfinite, 1ull);
    keys[e] = ((uint64_t)map << 48) | ((uint64_t)ma_image(u) << 16) | px;
  }
}

// sorted keys -> ranks2[map][pixel] = start + end + 1 of the key's tie group inside its map's segment
__global__ __launch_bounds__(256) void ma_ranks(const uint64_t* __restrict__ keys, uint32_t hw, uint32_t m,
                                                uint32_t* __restrict__ ranks2) {
  const uint32_t stride = gridDim.x * 256u;
  for (uint64_t e64 = (uint64_t)blockIdx.x * 256u + threadIdx.x; e64 < m; e64 += stride) {
    const uint32_t e = (uint32_t)e64;
    const uint32_t map = e / hw, i = e - map * hw;
    const uint64_t* seg = keys + (int64_t)map * hw;
    const uint64_t key = seg[i];
    const uint32_t img = ma_key_image(key);
    uint32_t start = i, end = i + 1;
    if (i > 0 && ma_key_image(seg[i - 1]) == img) {  // first position in [0, i) whose image is >= img
      uint32_t lo = 0, hi = i - 1;                   // seg[hi] is known equal
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ma_key_image(seg[mid]) < img) lo = mid + 1;
        else hi = mid;
      }
      start = lo;
    }
    if (i + 1 < hw && ma_key_image(seg[i + 1]) == img) {  // first position in (i + 1, hw] whose image is > img
      uint32_t lo = i + 2, hi = hw;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (ma_key_image(seg[mid]) <= img) lo = mid + 1;
        else hi = mid;
      }
      end = lo;
    }
    ranks2[(int64_t)map * hw + (uint32_t)(key & 0xFFFFu)] = start + end + 1;
  }
}

struct MaSm {
  double d[4];
  long long l[4];
};
// 256 threads -> every thread the sum: the wave_sum tree, then waves 0..3 in order
__device__ __forceinline__ double ma_block_sum(double v, MaSm& sm) {
  v = mmr::wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm.d[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((sm.d[0] + sm.d[1]) + sm.d[2]) + sm.d[3];
  __syncthreads();
  return r;
}
__device__ __forceinline__ long long ma_block_sum(long long v, MaSm& sm) {
  v = mmr::wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm.l[threadIdx.x >> 6] = v;
  __syncthreads();
  const long long r = sm.l[0] + sm.l[1] + sm.l[2] + sm.l[3];
  __syncthreads();
  return r;
}

struct MaK {
  int nf;
  int k[MA_MAXF];
};

// workgroup `map`: thresholds, constant flag, mean, sum of squared deviations
__global__ __launch_bounds__(256) void ma_map_stats(const float* __restrict__ maps, int64_t ld,
                                                    const uint64_t* __restrict__ keys, int hw, const MaK ks,
                                                    float* __restrict__ thr, int32_t* __restrict__ constant,
                                                    double* __restrict__ mean, double* __restrict__ ssd) {
  __shared__ MaSm sm;
  const int map = blockIdx.x, tid = threadIdx.x;
  const uint64_t* seg = keys + (int64_t)map * hw;
  if (tid < ks.nf)
    reinterpret_cast<uint32_t*>(thr)[map * ks.nf + tid] = ma_image_bits(ma_key_image(seg[hw - ks.k[tid]]));
  if (tid == 64) constant[map] = ma_key_image(seg[0]) == ma_key_image(seg[hw - 1]);
  const float* x = maps + (int64_t)map * ld;
  double s = 0.0;
  for (int i = tid; i < hw; i += 256) s += (double)x[i];
  const double mu = ma_block_sum(s, sm) / (double)hw;
  double q = 0.0;
  for (int i = tid; i < hw; i += 256) {
    const double d = (double)x[i] - mu;
    q += d * d;
  }
  q = ma_block_sum(q, sm);
  if (tid == 0) {
    mean[map] = mu;
    ssd[map] = q;
  }
}

// workgroup `pair`
__global__ __launch_bounds__(256) void ma_pair(const float* __restrict__ maps, int64_t ld, int64_t n, int hw,
                                               const int64_t* __restrict__ pa, const int64_t* __restrict__ pb,
                                               const uint32_t* __restrict__ ranks2, const float* __restrict__ thr,
                                               const int32_t* __restrict__ constant, const double* __restrict__ mean,
                                               const double* __restrict__ ssd, int nf, double* __restrict__ pearson,
                                               double* __restrict__ spearman, int64_t* __restrict__ rank_sums,
                                               int64_t* __restrict__ inter_union, int32_t* __restrict__ skipped) {
  __shared__ MaSm sm;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t ia = pa[p], ib = pb[p];
  if (ia < 0 || ia >= n || ib < 0 || ib >= n) {  // uniform over the workgroup
    if (tid == 0) {
      skipped[p] = 1;
      pearson[p] = 0.0;
      spearman[p] = 0.0;
      for (int j = 0; j < 3; ++j) rank_sums[3 * (int64_t)p + j] = 0;
      for (int j = 0; j < 2 * nf; ++j) inter_union[(int64_t)p * 2 * nf + j] = 0;
    }
    return;
  }
  const float *xa = maps + ia * ld, *xb = maps + ib * ld;
  const uint32_t *ra = ranks2 + ia * hw, *rb = ranks2 + ib * hw;
  const double ma = mean[ia], mb = mean[ib];
  float ta[MA_MAXF], tb[MA_MAXF];
#pragma unroll
  for (int j = 0; j < MA_MAXF; ++j) {
    ta[j] = j < nf ? thr[ia * nf + j] : 0.0f;
    tb[j] = j < nf ? thr[ib * nf + j] : 0.0f;
  }
  double sab = 0.0;
  long long rab = 0, raa = 0, rbb = 0, in[MA_MAXF] = {0, 0, 0, 0}, un[MA_MAXF] = {0, 0, 0, 0};
  const long long centre = (long long)hw + 1;
  for (int i = tid; i < hw; i += 256) {
    const float a = xa[i], b = xb[i];
    sab += ((double)a - ma) * ((double)b - mb);
    const long long ca = (long long)ra[i] - centre, cb = (long long)rb[i] - centre;
    rab += ca * cb;
    raa += ca * ca;
    rbb += cb * cb;
#pragma unroll
    for (int j = 0; j < MA_MAXF; ++j) {
      const bool ina = a >= ta[j], inb = b >= tb[j];
      in[j] += ina && inb;
      un[j] += ina || inb;
    }
  }
  sab = ma_block_sum(sab, sm);
  rab = ma_block_sum(rab, sm);
  raa = ma_block_sum(raa, sm);
  rbb = ma_block_sum(rbb, sm);
#pragma unroll
  for (int j = 0; j < MA_MAXF; ++j) {
    in[j] = ma_block_sum(in[j], sm);
    un[j] = ma_block_sum(un[j], sm);
  }
  if (tid == 0) {
    const bool flat = constant[ia] || constant[ib];
    skipped[p] = 0;
    pearson[p] = flat ? 0.0 : sab / sqrt(ssd[ia] * ssd[ib]);
    spearman[p] = flat ? 0.0 : (double)rab / sqrt((double)raa * (double)rbb);
    rank_sums[3 * (int64_t)p + 0] = rab;
    rank_sums[3 * (int64_t)p + 1] = raa;
    rank_sums[3 * (int64_t)p + 2] = rbb;
#pragma unroll
    for (int j = 0; j < MA_MAXF; ++j)
      if (j < nf) {
        inter_union[((int64_t)p * nf + j) * 2 + 0] = in[j];
        inter_union[((int64_t)p * nf + j) * 2 + 1] = un[j];
      }
  }
}

struct MaWork {
  CeSort sort;
  int64_t bytes;
};
inline MaWork ma_layout(int64_t n, int64_t hw, void* work) {
  MaWork w;
  char* p = (char*)work;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* at = p + off;
    off += mmr::round_up(bytes, 256);
    return at;
  };
  w.sort = ce_sort_layout(n * hw, take);
  w.bytes = off;
  return w;
}
inline bool ma_shape_ok(int64_t n, int32_t hw) {
  return n >= 1 && n <= 65536 && hw >= 1 && hw <= 65536 && n * (int64_t)hw < ((int64_t)1 << 31);
}

}  // namespace

extern "C" {

int64_t mmr_map_alignment_work_bytes(int64_t n, int32_t hw) {
  if (!ma_shape_ok(n, hw)) return 0;
  return ma_layout(n, hw, nullptr).bytes;
}

mmr_status mmr_map_alignment(const float* maps, int64_t ld, int64_t n, int32_t hw, const int64_t* pa,
                             const int64_t* pb, int64_t p, int32_t nf, int32_t k0, int32_t k1, int32_t k2, int32_t k3,
                             uint32_t* ranks2, float* thresholds, int32_t* constant, double* mean, double* ssd,
                             double* pearson, double* spearman, int64_t* rank_sums, int64_t* inter_union,
                             int32_t* skipped, int64_t* nonfinite, void* work, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(n >= 1 && n <= 65536, "mmr_map_alignment: N = %lld outside 1..65536", (long long)n);
  MMR_REQUIRE(hw >= 1 && hw <= 65536, "mmr_map_alignment: HW = %d outside 1..65536", hw);
  MMR_REQUIRE(ma_shape_ok(n, hw), "mmr_map_alignment: N * HW = %lld x %d does not fit 2^31 - 1 keys", (long long)n, hw);
  MMR_REQUIRE(ld >= hw, "mmr_map_alignment: map stride %lld < HW = %d", (long long)ld, hw);
  MMR_REQUIRE(p >= 0 && p <= 0x7FFFFFFF, "mmr_map_alignment: P = %lld outside 0..2^31 - 1", (long long)p);
  MMR_REQUIRE(nf >= 0 && nf <= MA_MAXF, "mmr_map_alignment: %d fractions outside 0..%d", nf, MA_MAXF);
  MaK ks;
  ks.nf = nf;
  const int32_t kk[MA_MAXF] = {k0, k1, k2, k3};
  for (int j = 0; j < MA_MAXF; ++j) {
    MMR_REQUIRE(j >= nf || (kk[j] >= 1 && kk[j] <= hw), "mmr_map_alignment: k[%d] = %d outside 1..HW = %d", j, kk[j],
                hw);
    ks.k[j] = j < nf ? kk[j] : 1;
  }
  MMR_REQUIRE(maps && (p == 0 || (pa && pb)), "mmr_map_alignment: NULL maps / pair lists");
  MMR_REQUIRE(ranks2 && constant && mean && ssd && nonfinite && (nf == 0 || thresholds),
              "mmr_map_alignment: NULL per-map output");
  MMR_REQUIRE(p == 0 || (pearson && spearman && rank_sums && skipped && (nf == 0 || inter_union)),
              "mmr_map_alignment: NULL per-pair output");
  MMR_REQUIRE(work && aligned16(work), "mmr_map_alignment: work is NULL or not 16-B aligned");
  hipStream_t st = mmr::as_stream(stream);
  const int64_t m = n * hw;
  const MaWork w = ma_layout(n, hw, work);
  MMR_CHECK_HIP(hipMemsetAsync(nonfinite, 0, sizeof(int64_t), st));
  const unsigned bgrid = (unsigned)(mmr::ceil_div(m, 256) < 2048 ? mmr::ceil_div(m, 256) : 2048);
  ma_build_keys<<<bgrid, 256, 0, st>>>((const uint32_t*)maps, ld, (uint32_t)hw, (uint32_t)m, w.sort.ka,
                                       (unsigned long long*)nonfinite);
  int nbits = 0;
  while (((int64_t)1 << nbits) < n) ++nbits;
  const uint64_t* sorted = ce_sort(w.sort.ka, w.sort.kb, m, 16, 48 + nbits, w.sort, st);
  ma_ranks<<<bgrid, 256, 0, st>>>(sorted, (uint32_t)hw, (uint32_t)m, ranks2);
  ma_map_stats<<<dim3((unsigned)n), 256, 0, st>>>(maps, ld, sorted, hw, ks, thresholds, constant, mean, ssd);
  if (p > 0)
    ma_pair<<<dim3((unsigned)p), 256, 0, st>>>(maps, ld, n, hw, pa, pb, ranks2, thresholds, constant, mean, ssd, nf,
                                               pearson, spearman, rank_sums, inter_union, skipped);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

}  // extern "C"
