// The stable LSD radix sort of u64 keys that the classifier evaluation (cls_eval.hip) and the map alignment
// (map_align.hip) share: 8-bit digits, one wave (a 64-thread workgroup) per contiguous chunk of <= `per` keys:
// ce_hist (LDS histogram of the chunk) -> ce_hist_scan (one workgroup per digit value: exclusive scan over the
// chunks, digit totals) -> ce_scatter (digit bases = scan of the totals; per 64 keys the lanes of equal digit find
// each other with 8 ballots, rank = popcount below, the group's first lane advances the LDS base: stable).
// Included inside the including file's anonymous namespace, after common.h.
#pragma once

constexpr int CE_WMAX = 4096;  // sort chunks (waves) per pass at most

__global__ __launch_bounds__(64) void ce_hist(const uint64_t* __restrict__ in, int64_t m, int64_t per, int shift,
                                              uint32_t* __restrict__ hist, int W) {
  __shared__ uint32_t h[256];
  const int lane = threadIdx.x, w = blockIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) h[lane + 64 * j] = 0;
  __syncthreads();
  const int64_t begin = (int64_t)w * per, end = begin + per < m ? begin + per : m;
  for (int64_t i = begin + lane; i < end; i += 256) {  // 4 keys' loads in flight
    uint64_t k[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) k[u] = i + 64 * u < end ? in[i + 64 * u] : 0ull;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + 64 * u < end) atomicAdd(&h[(uint32_t)(k[u] >> shift) & 255u], 1u);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) hist[(int64_t)(lane + 64 * j) * W + w] = h[lane + 64 * j];
}

__device__ __forceinline__ uint32_t ce_wave_incl(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// workgroup `bin`: hist[bin][0 .. W) -> its exclusive scan, totals[bin] = the sum
__global__ __launch_bounds__(256) void ce_hist_scan(uint32_t* __restrict__ hist, int W, uint32_t* __restrict__ totals) {
  __shared__ uint32_t wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* row = hist + (int64_t)blockIdx.x * W;
  const int ept = (W + 255) / 256;  // <= CE_WMAX / 256: a thread's entries stay in registers
  const int i0 = tid * ept < W ? tid * ept : W, i1 = i0 + ept < W ? i0 + ept : W;
  uint32_t v[CE_WMAX / 256], s = 0;
#pragma unroll
  for (int j = 0; j < CE_WMAX / 256; ++j) {
    v[j] = i0 + j < i1 ? row[i0 + j] : 0u;
    s += v[j];
  }
  const uint32_t incl = ce_wave_incl(s, lane);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t run = incl - s, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) run += wsum[w];
    total += wsum[w];
  }
#pragma unroll
  for (int j = 0; j < CE_WMAX / 256; ++j) {
    if (i0 + j < i1) row[i0 + j] = run;
    run += v[j];
  }
  if (tid == 0) totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(64) void ce_scatter(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int64_t m,
                                                 int64_t per, int shift, const uint32_t* __restrict__ hist,
                                                 const uint32_t* __restrict__ totals, int W) {
  __shared__ uint32_t base[256];
  const int lane = threadIdx.x, w = blockIdx.x;
  {  // lane: digits 4 lane .. 4 lane + 3
    uint32_t t[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[j] = totals[4 * lane + j];
      s += t[j];
    }
    uint32_t b = ce_wave_incl(s, lane) - s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      base[4 * lane + j] = b + hist[(int64_t)(4 * lane + j) * W + w];
      b += t[j];
    }
  }
  __syncthreads();
  const int64_t begin = (int64_t)w * per, end = begin + per < m ? begin + per : m;
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t ahead = begin + lane < end ? in[begin + lane] : 0ull;  // the next round's key, loaded a round early
  for (int64_t i0 = begin; i0 < end; i0 += 64) {  // uniform trip count: the barriers are met by every lane
    const int64_t i = i0 + lane;
    const bool valid = i < end;
    const uint64_t key = ahead;
    ahead = i + 64 < end ? in[i + 64] : 0ull;
    const uint32_t d = (uint32_t)(key >> shift) & 255u;
    uint64_t same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const uint32_t rank = __popcll(same & below), cnt = __popcll(same);
    const uint32_t pos = valid ? base[d] : 0u;
    __syncthreads();
    if (valid && rank == 0) base[d] = pos + cnt;
    __syncthreads();
    if (valid && (int64_t)pos + rank < m) out[pos + rank] = key;
  }
}

// the sort's scratch: two key arrays of m keys, the (digit, chunk) histogram and the digit totals
struct CeSort {
  uint64_t *ka, *kb;
  uint32_t *hist, *totals;
  int64_t per;
  int W;
};
// take(bytes) -> the next piece of the caller's work buffer
template <class Take>
inline CeSort ce_sort_layout(int64_t m, Take&& take) {
  CeSort w;
  w.per = mmr::round_up(mmr::ceil_div(m, CE_WMAX), 64);
  w.W = (int)mmr::ceil_div(m, w.per);
  w.ka = (uint64_t*)take(m * 8);
  w.kb = (uint64_t*)take(m * 8);
  w.hist = (uint32_t*)take((int64_t)256 * w.W * 4);
  w.totals = (uint32_t*)take(256 * 4);
  return w;
}

// ascending sort of keys[0 .. m) over bits [lo, hi); returns the array that holds the result (keys or alt)
inline uint64_t* ce_sort(uint64_t* keys, uint64_t* alt, int64_t m, int lo, int hi, const CeSort& w, hipStream_t st) {
  for (int shift = lo; shift < hi; shift += 8) {
    ce_hist<<<dim3((unsigned)w.W), 64, 0, st>>>(keys, m, w.per, shift, w.hist, w.W);
    ce_hist_scan<<<256, 256, 0, st>>>(w.hist, w.W, w.totals);
    ce_scatter<<<dim3((unsigned)w.W), 64, 0, st>>>(keys, alt, m, w.per, shift, w.hist, w.totals, w.W);
    uint64_t* t = keys;
    keys = alt;
    alt = t;
  }
  return keys;
}
