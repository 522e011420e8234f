// Classifier evaluation (src/Evaluate/eval_on_test.py; Trainner/train.py:621-681): per class and for the N*C
// flattened (score, label) pairs ("micro") the exact ROC / PR curve sums, the best-F1 threshold
// (_find_best_thresholds) and the confusion counts of `score > threshold` — on device, from (N, C) f32 scores and
// (N,) uint64 label bitsets.  Every output is an integer, an f64 sum in a fixed tree order or an argmax under a
// total order: no float atomics, identical bytes run to run.  The floats (AUROC, AP, precision ...) are derived
// from them on the host in f64 (metrics.classification_metrics).
//
// Keys.  ce_build_keys writes one u64 per (sample, class):  [class : bits 33..38 | image : bits 1..32 | label :
// bit 0], image = ~(order-preserving u32 image of the f32 score, -0 canonicalised to +0): an ascending integer
// sort lists scores in DESCENDING order, and all ordering comes from integer compares on the bit pattern
// (denormals stay distinct whatever the float mode).  Non-finite scores are counted (integer atomic) and
// reported; the caller raises.
//
// Sort.  ONE stable LSD radix sort serves both orders: after the passes over the image bits [1, 33) the N C keys
// are the micro segment (the curve kernels compare the 32 image bits only, the class field rides along); one more
// pass over the class bits [33, 33 + ceil(log2 C)) then leaves every class a contiguous sorted segment — 5 passes
// instead of the 4 + 5 of two sorts, and no second key array.  ce_sort: 8-bit digits, one wave (a 64-thread
// workgroup) per contiguous chunk of <= `per` keys: ce_hist (LDS histogram of the chunk) -> ce_hist_scan (one
// workgroup per digit value: exclusive scan over the chunks, digit totals) -> ce_scatter (digit bases = scan of
// the totals; per 64 keys the lanes of equal digit find each other with 8 ballots, rank = popcount below, the
// group's first lane advances the LDS base: stable).  The label bit is not sorted: the order inside a tie group
// reaches no output.  Every class has exactly N keys, so after the last pass class c is the segment
// [c N, (c + 1) N).
//
// Curve.  Per segment (C segments of N, or 1 of N C), tiles of 1024 keys: ce_tile_agg reduces each tile to an
// aggregate of the segmented-scan monoid (tp = labels, flag = a tie group starts, dtp / cnt = labels / keys since
// the last start), ce_tile_scan scans the aggregates per segment (and leaves P = the segment's positives),
// ce_tile_curve redoes the tile's scan from its prefix: at every tie-group end tp, fp = rank - tp, dtp, dfp are
// exact integers and
//   A     += dfp (2 (tp - dtp) + dtp)                      (int64; AUROC = A / (2 P Nn))
//   ap    += dtp * (tp / (tp + fp))                        (f64; AP = ap / P)
//   f1     = (2 p r) / ((p + r) + 1e-8), p = tp / (tp + fp), r = P ? tp / P : 1    (each op rounded on its own:
//            fp contraction is off for this file) — argmax under (f1 desc, score asc), the reference's
//            f1.argmax() over ascending thresholds
// are reduced thread -> wave (xor butterfly) -> workgroup -> tile partial; ce_seg_finish reduces a segment's
// partials in a fixed order.  ce_confusion: one pass over the unsorted scores against the thresholds (the best-F1
// ones or the caller's), lane = class, integer compare of the images; per-workgroup counts, summed by
// ce_confusion_finish (atomics on the 3 (C + 1) result words cost more than the whole pass).
#include "common.h"

#pragma clang fp contract(off)

namespace {

using mmr::aligned16;

constexpr int CE_TILE = 1024;  // curve tile: 256 threads x 4 consecutive keys
constexpr int CE_MAXC = 64;

// ~(ascending image): larger score -> smaller image; -0 -> +0
__device__ __forceinline__ uint32_t ce_image(uint32_t u) {
  if ((u << 1) == 0) u = 0;
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}
__device__ __forceinline__ uint32_t ce_image_bits(uint32_t img) {  // the f32 bit pattern of an image
  const uint32_t asc = ~img;
  return (asc & 0x80000000u) ? (asc ^ 0x80000000u) : ~asc;
}

__global__ __launch_bounds__(256) void ce_build_keys(const uint32_t* __restrict__ s, int64_t ld,
                                                     const uint64_t* __restrict__ bits, uint32_t c, uint32_t m,
                                                     uint64_t* __restrict__ keys,
                                                     unsigned long long* __restrict__ nonfinite) {
  const uint32_t stride = gridDim.x * 256u;
  for (uint64_t e64 = (uint64_t)blockIdx.x * 256u + threadIdx.x; e64 < m; e64 += stride) {
    const uint32_t e = (uint32_t)e64;
    const uint32_t row = e / c, col = e - row * c;
    const uint32_t u = s[(int64_t)row * ld + col];
    if ((u & 0x7F800000u) == 0x7F800000u) atomicAdd(nonfinite, 1ull);
    keys[e] = ((uint64_t)col << 33) | ((uint64_t)ce_image(u) << 1) | ((bits[row] >> col) & 1ull);
  }
}

// ------------------------------------------------------------------------------------------------ radix sort
#include "radix_sort.h"

// ------------------------------------------------------------------------------------------------ curve
// the segmented-scan monoid: tp = labels, flag = a group starts, dtp / cnt = labels / keys since the last start
struct CeAgg {
  int tp, flag, dtp, cnt;
};
__device__ __forceinline__ CeAgg ce_id() { return CeAgg{0, 0, 0, 0}; }
__device__ __forceinline__ CeAgg ce_comb(const CeAgg a, const CeAgg b) {
  return CeAgg{a.tp + b.tp, a.flag | b.flag, b.flag ? b.dtp : a.dtp + b.dtp, b.flag ? b.cnt : a.cnt + b.cnt};
}
__device__ __forceinline__ CeAgg ce_shfl_up(const CeAgg v, int off) {
  return CeAgg{__shfl_up(v.tp, off, 64), __shfl_up(v.flag, off, 64), __shfl_up(v.dtp, off, 64),
               __shfl_up(v.cnt, off, 64)};
}
// 256 threads: the exclusive prefix of each thread's aggregate and the workgroup's total; sm: 4 entries
__device__ __forceinline__ CeAgg ce_block_excl(const CeAgg t, CeAgg* sm, CeAgg& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  CeAgg incl = t;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const CeAgg o = ce_shfl_up(incl, off);
    if (lane >= off) incl = ce_comb(o, incl);
  }
  CeAgg ex = ce_shfl_up(incl, 1);
  if (lane == 0) ex = ce_id();
  if (lane == 63) sm[wave] = incl;
  __syncthreads();
  CeAgg wp = ce_id();
  total = ce_id();
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const CeAgg a = sm[w];
    if (w < wave) wp = ce_comb(wp, a);
    total = ce_comb(total, a);
  }
  __syncthreads();
  return ce_comb(wp, ex);
}

// a thread's 4 consecutive keys of tile t of a segment of L keys at p
struct CeItems {
  uint64_t key[4];
  bool valid[4], start[4], end[4];
  int64_t j0;
};
__device__ __forceinline__ CeItems ce_load(const uint64_t* __restrict__ p, int64_t L, int64_t t) {
  constexpr uint64_t NONE = ~0ull;  // no group key: a group key is the 32 image bits (the class field is not compared)
  CeItems it;
  it.j0 = t * CE_TILE + (int64_t)threadIdx.x * 4;
  uint64_t g[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    it.valid[k] = it.j0 + k < L;
    it.key[k] = it.valid[k] ? p[it.j0 + k] : 0ull;
    g[k] = it.valid[k] ? (uint32_t)(it.key[k] >> 1) : NONE;
  }
  const uint64_t prev = (it.j0 > 0 && it.j0 - 1 < L) ? (uint32_t)(p[it.j0 - 1] >> 1) : NONE;
  const uint64_t next = it.j0 + 4 < L ? (uint32_t)(p[it.j0 + 4] >> 1) : NONE;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    it.start[k] = it.valid[k] && g[k] != (k ? g[k - 1] : prev);
    it.end[k] = it.valid[k] && g[k] != (k < 3 ? g[k + 1] : next);
  }
  return it;
}
__device__ __forceinline__ CeAgg ce_elem(const CeItems& it, int k) {
  const int lab = (int)(it.key[k] & 1ull);
  return CeAgg{lab, it.start[k] ? 1 : 0, lab, 1};
}

__global__ __launch_bounds__(256) void ce_tile_agg(const uint64_t* __restrict__ keys, int64_t L, int64_t T,
                                                   CeAgg* __restrict__ tagg) {
  __shared__ CeAgg sm[4];
  const int64_t seg = blockIdx.x / T, t = blockIdx.x % T;
  const CeItems it = ce_load(keys + seg * L, L, t);
  CeAgg a = ce_id();
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (it.valid[k]) a = ce_comb(a, ce_elem(it, k));
  CeAgg total;
  (void)ce_block_excl(a, sm, total);
  if (threadIdx.x == 0) tagg[blockIdx.x] = total;
}

// workgroup `seg`: the exclusive scan of its T tile aggregates, segp[seg] = the segment's positives
__global__ __launch_bounds__(256) void ce_tile_scan(const CeAgg* __restrict__ tagg, int64_t T, CeAgg* __restrict__ tpre,
                                                    int32_t* __restrict__ segp) {
  __shared__ CeAgg sm[4];
  const int64_t o = (int64_t)blockIdx.x * T;
  CeAgg carry = ce_id();
  for (int64_t t0 = 0; t0 < T; t0 += 256) {  // uniform trip count
    const int64_t t = t0 + threadIdx.x;
    const CeAgg a = t < T ? tagg[o + t] : ce_id();
    CeAgg total;
    const CeAgg ex = ce_block_excl(a, sm, total);
    if (t < T) tpre[o + t] = ce_comb(carry, ex);
    carry = ce_comb(carry, total);
  }
  if (threadIdx.x == 0) segp[blockIdx.x] = carry.tp;
}

struct CePart {
  long long a;
  double ap, f1;
  uint32_t img;
  int nd;
};
// (f1 desc, score asc = image desc); "none" is f1 = -1
__device__ __forceinline__ bool ce_better(double f, uint32_t i, double f2, uint32_t i2) {
  return f > f2 || (f == f2 && i > i2);
}
// 256 threads -> thread 0 holds the workgroup's partial; sums in the wave_sum tree, then waves 0..3 in order
__device__ __forceinline__ CePart ce_block_reduce(CePart v, CePart* sm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v.a = mmr::wave_sum(v.a);
  v.ap = mmr::wave_sum(v.ap);
  v.nd = mmr::wave_sum(v.nd);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double f2 = __shfl_xor(v.f1, m, 64);
    const uint32_t i2 = __shfl_xor(v.img, m, 64);
    if (ce_better(f2, i2, v.f1, v.img)) {
      v.f1 = f2;
      v.img = i2;
    }
  }
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  CePart r = sm[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const CePart b = sm[w];
    r.a += b.a;
    r.ap += b.ap;
    r.nd += b.nd;
    if (ce_better(b.f1, b.img, r.f1, r.img)) {
      r.f1 = b.f1;
      r.img = b.img;
    }
  }
  return r;
}

__global__ __launch_bounds__(256) void ce_tile_curve(const uint64_t* __restrict__ keys, int64_t L, int64_t T,
                                                     const CeAgg* __restrict__ tpre, const int32_t* __restrict__ segp,
                                                     CePart* __restrict__ part) {
  __shared__ CeAgg sm[4];
  __shared__ CePart smp[4];
  const int64_t seg = blockIdx.x / T, t = blockIdx.x % T;
  const CeItems it = ce_load(keys + seg * L, L, t);
  CeAgg a = ce_id();
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (it.valid[k]) a = ce_comb(a, ce_elem(it, k));
  CeAgg total;
  CeAgg run = ce_comb(tpre[blockIdx.x], ce_block_excl(a, sm, total));
  const int P = segp[seg];
  CePart v{0, 0.0, -1.0, 0u, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!it.valid[k]) continue;
    run = ce_comb(run, ce_elem(it, k));
    if (!it.end[k]) continue;
    const int64_t n = it.j0 + k + 1;  // tp + fp: the keys ranked at or above this score
    const int tp = run.tp, dtp = run.dtp, dfp = run.cnt - run.dtp;
    v.a += (long long)dfp * (2ll * (tp - dtp) + dtp);
    const double p = (double)tp / (double)n;
    v.ap += (double)dtp * p;
    const double r = P ? (double)tp / (double)P : 1.0;
    const double f1 = (2.0 * p * r) / ((p + r) + 1e-8);
    const uint32_t img = (uint32_t)(it.key[k] >> 1);
    if (ce_better(f1, img, v.f1, v.img)) {
      v.f1 = f1;
      v.img = img;
    }
    ++v.nd;
  }
  const CePart r = ce_block_reduce(v, smp);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// workgroup `seg`: its T tile partials (thread i: tiles i, i + 256, ... in order) -> result row row0 + seg
__global__ __launch_bounds__(256) void ce_seg_finish(const CePart* __restrict__ part, int64_t T, int64_t L,
                                                     const int32_t* __restrict__ segp, int row0,
                                                     int64_t* __restrict__ counts, double* __restrict__ ap_sum,
                                                     uint32_t* __restrict__ best_thr, double* __restrict__ best_f1) {
  __shared__ CePart smp[4];
  const CePart* p = part + (int64_t)blockIdx.x * T;
  CePart v{0, 0.0, -1.0, 0u, 0};
  for (int64_t t = threadIdx.x; t < T; t += 256) {
    const CePart b = p[t];
    v.a += b.a;
    v.ap += b.ap;
    v.nd += b.nd;
    if (ce_better(b.f1, b.img, v.f1, v.img)) {
      v.f1 = b.f1;
      v.img = b.img;
    }
  }
  const CePart r = ce_block_reduce(v, smp);
  if (threadIdx.x == 0) {
    const int row = row0 + blockIdx.x;
    const int64_t P = segp[blockIdx.x];
    counts[4 * row + 0] = P;
    counts[4 * row + 1] = L - P;
    counts[4 * row + 2] = r.a;
    counts[4 * row + 3] = r.nd;
    ap_sum[row] = r.ap;
    best_thr[row] = ce_image_bits(r.img);
    best_f1[row] = r.f1;
  }
}

// lane = class; wave g of the grid takes rows g, g + G, ...; part [workgroup][tp, fp, fn][64] = its counts
__global__ __launch_bounds__(256) void ce_confusion(const uint32_t* __restrict__ s, int64_t ld,
                                                    const uint64_t* __restrict__ bits, int64_t n, int c,
                                                    const uint32_t* __restrict__ thr, uint32_t* __restrict__ part) {
  __shared__ uint32_t sm[4][3][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = lane < c;
  const uint32_t timg = live ? ce_image(thr[lane]) : 0u;
  uint32_t tp = 0, fp = 0, fn = 0;
  const int64_t G = (int64_t)gridDim.x * 4;
  for (int64_t row0 = (int64_t)blockIdx.x * 4 + wave; row0 < n; row0 += 4 * G) {  // 4 rows' loads in flight
    uint32_t u[4];
    uint64_t b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t row = row0 + k * G;
      const bool ok = live && row < n;
      u[k] = ok ? s[row * ld + lane] : 0u;
      b[k] = ok ? bits[row] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = live && row0 + k * G < n;
      const bool pred = ok && ce_image(u[k]) < timg;  // score > threshold
      const bool lab = (b[k] >> lane) & 1ull;
      tp += pred && lab;
      fp += pred && !lab;
      fn += ok && !pred && lab;
    }
  }
  sm[wave][0][lane] = tp;
  sm[wave][1][lane] = fp;
  sm[wave][2][lane] = fn;
  __syncthreads();
  if (wave < 3)
    part[((int64_t)blockIdx.x * 3 + wave) * 64 + lane] =
        sm[0][wave][lane] + sm[1][wave][lane] + sm[2][wave][lane] + sm[3][wave][lane];
}

// workgroup k (tp, fp, fn): the nb workgroup partials of ce_confusion -> conf (c + 1, 3) int64, row c = the sum
// over the classes; lane = class, wave w of 16 adds the partials w, w + 16, ...
__global__ __launch_bounds__(1024) void ce_confusion_finish(const uint32_t* __restrict__ part, int nb, int c,
                                                            int64_t* __restrict__ conf) {
  __shared__ long long sm[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = blockIdx.x;
  long long v = 0;
  for (int b = wave; b < nb; b += 64) {  // 4 partials' loads in flight
    uint32_t x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = b + 16 * u < nb ? part[((int64_t)(b + 16 * u) * 3 + k) * 64 + lane] : 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) v += x[u];
  }
  sm[wave][lane] = v;
  __syncthreads();
  if (wave == 0) {
    v = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) v += sm[w][lane];  // lanes >= c counted nothing
    if (lane < c) conf[3 * lane + k] = v;
    const long long all = mmr::wave_sum(v);
    if (lane == 0) conf[3 * c + k] = all;
  }
}

// ------------------------------------------------------------------------------------------------ host
struct CeWork {
  CeSort sort;
  CeAgg *tagg, *tpre;
  int32_t* segp;
  CePart* part;
  uint32_t* cpart;
  int64_t tiles, bytes;
  int cgrid;
};
inline CeWork ce_layout(int64_t n, int64_t c, void* work) {
  const int64_t m = n * c;
  CeWork w;
  const int64_t tc = c * mmr::ceil_div(n, CE_TILE), tm = mmr::ceil_div(m, CE_TILE);
  w.tiles = tc > tm ? tc : tm;
  char* p = (char*)work;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* at = p + off;
    off += mmr::round_up(bytes, 256);
    return at;
  };
  w.sort = ce_sort_layout(m, take);
  w.tagg = (CeAgg*)take(w.tiles * (int64_t)sizeof(CeAgg));
  w.tpre = (CeAgg*)take(w.tiles * (int64_t)sizeof(CeAgg));
  w.segp = (int32_t*)take(CE_MAXC * 4);
  w.part = (CePart*)take(w.tiles * (int64_t)sizeof(CePart));
  w.cgrid = (int)(mmr::ceil_div(n, 4) < 1024 ? mmr::ceil_div(n, 4) : 1024);
  w.cpart = (uint32_t*)take((int64_t)w.cgrid * 3 * 64 * 4);
  w.bytes = off;
  return w;
}

// S segments of L sorted keys -> result rows row0 .. row0 + S - 1
void ce_curve(const uint64_t* keys, int64_t S, int64_t L, int row0, const CeWork& w, int64_t* counts, double* ap_sum,
              float* best_thr, double* best_f1, hipStream_t st) {
  const int64_t T = mmr::ceil_div(L, CE_TILE);
  const dim3 grid((unsigned)(S * T));
  ce_tile_agg<<<grid, 256, 0, st>>>(keys, L, T, w.tagg);
  ce_tile_scan<<<dim3((unsigned)S), 256, 0, st>>>(w.tagg, T, w.tpre, w.segp);
  ce_tile_curve<<<grid, 256, 0, st>>>(keys, L, T, w.tpre, w.segp, w.part);
  ce_seg_finish<<<dim3((unsigned)S), 256, 0, st>>>(w.part, T, L, w.segp, row0, counts, ap_sum, (uint32_t*)best_thr,
                                                   best_f1);
}

inline bool ce_shape_ok(int64_t n, int32_t c) {
  return n >= 1 && c >= 1 && c <= CE_MAXC && n < ((int64_t)1 << 31) && n * (int64_t)c < ((int64_t)1 << 31);
}

}  // namespace

extern "C" {

int64_t mmr_cls_eval_work_bytes(int64_t n, int32_t c) {
  if (!ce_shape_ok(n, c)) return 0;
  return ce_layout(n, c, nullptr).bytes;
}

mmr_status mmr_cls_eval(const float* scores, int64_t lds, const uint64_t* label_bits, int64_t n, int32_t c,
                        const float* thresholds, int64_t* counts, double* ap_sum, float* best_thr, double* best_f1,
                        int64_t* confusion, int64_t* nonfinite, void* work, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(n >= 1, "mmr_cls_eval: n = %lld < 1", (long long)n);
  MMR_REQUIRE(c >= 1 && c <= CE_MAXC, "mmr_cls_eval: c = %d outside 1..%d (label sets are uint64)", c, CE_MAXC);
  MMR_REQUIRE(ce_shape_ok(n, c), "mmr_cls_eval: n * c = %lld x %d does not fit 2^31 - 1 keys", (long long)n, c);
  MMR_REQUIRE(lds >= c, "mmr_cls_eval: row stride %lld < c = %d", (long long)lds, c);
  MMR_REQUIRE(scores && label_bits, "mmr_cls_eval: NULL scores / label_bits");
  MMR_REQUIRE(counts && ap_sum && best_thr && best_f1 && confusion && nonfinite, "mmr_cls_eval: NULL output");
  MMR_REQUIRE(work && aligned16(work), "mmr_cls_eval: work is NULL or not 16-B aligned");
  hipStream_t st = mmr::as_stream(stream);
  const int64_t m = n * c;
  const CeWork w = ce_layout(n, c, work);
  MMR_CHECK_HIP(hipMemsetAsync(nonfinite, 0, sizeof(int64_t), st));
  const unsigned bgrid = (unsigned)(mmr::ceil_div(m, 256) < 2048 ? mmr::ceil_div(m, 256) : 2048);
  ce_build_keys<<<bgrid, 256, 0, st>>>((const uint32_t*)scores, lds, label_bits, (uint32_t)c, (uint32_t)m, w.sort.ka,
                                       (unsigned long long*)nonfinite);
  int cbits = 0;
  while ((1 << cbits) < c) ++cbits;
  uint64_t* sm = ce_sort(w.sort.ka, w.sort.kb, m, 1, 33, w.sort, st);  // by score: the micro segment
  ce_curve(sm, 1, m, c, w, counts, ap_sum, best_thr, best_f1, st);
  const uint64_t* sc = ce_sort(sm, sm == w.sort.ka ? w.sort.kb : w.sort.ka, m, 33, 33 + cbits, w.sort, st);  // stable: by class, then score
  ce_curve(sc, c, n, 0, w, counts, ap_sum, best_thr, best_f1, st);
  ce_confusion<<<dim3((unsigned)w.cgrid), 256, 0, st>>>((const uint32_t*)scores, lds, label_bits, n, c,
                                                        (const uint32_t*)(thresholds ? thresholds : best_thr), w.cpart);
  ce_confusion_finish<<<3, 1024, 0, st>>>(w.cpart, w.cgrid, c, confusion);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

}  // extern "C"
