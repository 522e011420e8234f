// Classification head on the joint embedding and the predict() tail (src/Model/model.py:271-277, 481,
// 491-537), eval: logits = W2 GELU_erf(W1 x + b1) + b2 (the Dropouts are identities), probs = sigmoid(logits),
// preds = probs >= threshold, top-K labels per query.  One precision in every tower mode, the rules of
// linear_x3 / x3_mlp: f32 activations, both contractions on bf16x3 MFMA (hi.hi + hi.lo + lo.hi, f32
// accumulate), mmr::gelu_erf.  D -> 4D -> C with C small (43 at the reference's configs): two mmr_linear_x3
// launches would write and re-read a (B, 4D) f32 hidden and need C % 32 == 0.
//
// cls_head_partial: grid (ceil(B / 32) row tiles) x (NS hidden slabs), one 32-wide hidden tile per wave.
//   The 32 x D x tile is split once per workgroup into hi / lo B-fragment images in LDS (D <= 1024: <= 128 KB).
//   fc1 in the C^T orientation on v_mfma_f32_32x32x16_bf16: A = the wave's 32 W1 rows, pre-split and stored
//   in fragment order (one coalesced 1-KB load per fragment, straight from L2 into registers, a 4-k-step
//   chunk in flight while the previous one is multiplied), bias in the accumulator.  After GELU the hidden is
//   split in registers into the hi / lo B operands of fc2 (the x3_mlp.hip hand-off; W2 stored under the
//   mmr::w2_hidden k-permutation), which accumulates logits^T [Cp][32 rows].  The waves' partial tiles are
//   summed in LDS in wave order and written to the workspace [NS][B][Cp].  Rows >= B are clamped on load
//   and never stored.  No atomics; the slab partition depends on (D, H) only, so a query's logits have the
//   same bits whatever else is in the batch.
// cls_head_finish: one wave per query: slab partials summed in slab order + b2 -> logits; probs =
//   1 / (1 + exp(-logit)) (mmr::exp_acc, IEEE divide); preds; top-K by rank-by-counting on (prob desc,
//   class asc) with the row's probabilities in registers (lane l holds classes l, l + 64, ...).
// Geometries off the fused kernel (D % 128, D > 1024, H != 4D) run mmr_linear_x3 / mmr_linear_f32 twice (W2
// zero-padded to Cp rows) into an NS = 1 workspace, then the same finish.
#include "common.h"

namespace {

using mmr::aligned16;
using mmr::bf16x8;
using mmr::f32x16;
using mmr::f32x4;
using mmr::split2;

constexpr int CLS_MAX_C = 256;
enum { CLS_NONE = -1, CLS_FUSED = 0, CLS_CHAIN_X3 = 1, CLS_CHAIN_F32 = 2 };

inline int cls_cp(int c) { return (c + 31) / 32 * 32; }
// fc2 output tiles the fused kernel is built for (W2 image rows = 32 nut, zero past C)
inline int cls_nut(int c) { return c <= 64 ? 2 : (c <= 128 ? 4 : 8); }
inline int cls_route(int d, int h, int c) {
  if (d <= 0 || h <= 0 || c < 1 || c > CLS_MAX_C) return CLS_NONE;
  if (d % 128 == 0 && d <= 1024 && h == 4 * d) return CLS_FUSED;
  if (d % 128 == 0 && h % 128 == 0) return CLS_CHAIN_X3;
  if (d % 16 == 0 && h % 32 == 0) return CLS_CHAIN_F32;
  return CLS_NONE;
}
// 32-wide hidden tiles (= waves) per slab: a function of D alone.  H / 32 = 16 (D / 128) tiles; 3 per slab
// where that divides (D = 768: 32 slabs, B = 256 -> 8 x 32 workgroups on 256 CUs), else 4
inline int cls_slab_tiles(int d) { return (d / 128) % 3 == 0 ? 3 : 4; }
inline int cls_slabs(int d) { return d / 8 / cls_slab_tiles(d); }
inline int64_t cls_part_bytes(int64_t b, int cp) { return mmr::round_up(b * cp * 4, 256); }

// Fused images, both in MFMA A-fragment order (fragment = [hi 64 lanes x 8 | lo 64 lanes x 8] bf16, lane
// (r, hf) = (lane % 32, lane / 32)):
//   W1: fragment (j, ks), j < H / 32, ks < D / 16: element e of lane = W1[32 j + r][16 ks + 8 hf + e]
//   W2: fragment (j, s2, u), s2 < 2, u < nut: element e of lane = W2[32 u + r][32 j + 16 s2 + w2_hidden(8 hf + e)]
//       (rows >= C zero)
__global__ __launch_bounds__(256) void cls_pack_fused(const float* __restrict__ w1, const float* __restrict__ w2,
                                                      uint16_t* __restrict__ img, int d, int h, int c, int nut) {
  const int64_t n1 = (int64_t)h * d * 2, n2 = (int64_t)h * nut * 64;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n1 + n2) return;
  const int64_t i2 = i < n1 ? i : i - n1;
  const int e = (int)(i2 & 7), lane = (int)(i2 >> 3) & 63, part = (int)(i2 >> 9) & 1;
  const int64_t f = i2 >> 10;
  const int r = lane & 31, hf = lane >> 5;
  float v;
  if (i < n1) {
    const int ks1 = d / 16, j = (int)(f / ks1), ks = (int)(f % ks1);
    v = w1[(int64_t)(32 * j + r) * d + 16 * ks + 8 * hf + e];
  } else {
    const int u = (int)(f % nut), s2 = (int)(f / nut) & 1, j = (int)(f / (2 * nut));
    const int cls = 32 * u + r, hid = 32 * j + 16 * s2 + mmr::w2_hidden(8 * hf + e);
    v = cls < c ? w2[(int64_t)cls * h + hid] : 0.f;
  }
  const uint16_t hi = mmr::f2bf(v);
  img[i] = part ? mmr::f2bf(v - mmr::bf2f(hi)) : hi;
}

// Chain images: X3: bf16 [W1_hi [H][D] | W1_lo | W2_hi [Cp][H] | W2_lo]; else f32 [W1 | W2 [Cp][H]] (rows >= C zero)
template <bool X3>
__global__ __launch_bounds__(256) void cls_pack_chain(const float* __restrict__ w1, const float* __restrict__ w2,
                                                      void* __restrict__ img, int d, int h, int c, int cp) {
  const int64_t n1 = (int64_t)h * d, n2 = (int64_t)cp * h;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n1 + n2) return;
  const float v = i < n1 ? w1[i] : ((i - n1) / h < c ? w2[i - n1] : 0.f);
  if constexpr (X3) {
    uint16_t* o = (uint16_t*)img;
    const uint16_t hi = mmr::f2bf(v), lo = mmr::f2bf(v - mmr::bf2f(hi));
    if (i < n1) {
      o[i] = hi;
      o[n1 + i] = lo;
    } else {
      o[2 * n1 + (i - n1)] = hi;
      o[2 * n1 + n2 + (i - n1)] = lo;
    }
  } else {
    ((float*)img)[i] = v;
  }
}

template <int NU>
__global__ __launch_bounds__(256) void cls_head_partial(const float* __restrict__ x, int64_t ldx,
                                                        const uint16_t* __restrict__ img,
                                                        const float* __restrict__ b1, float* __restrict__ work,
                                                        int nb, int d, int cp, int tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // x fragment images, then the reduction
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 31, hf = lane >> 5;
  const int nthr = blockDim.x;  // 64 tiles
  const int ks1 = d / 16;
  const int row0 = blockIdx.x * 32, slab = blockIdx.y;

  // x tile -> B fragments [ks][hi | lo][lane][8] (lane: row r, k = 16 ks + 8 hf ..+ 7); rows >= nb clamped
  for (int i = threadIdx.x; i < ks1 * 64; i += nthr) {
    const int ks = i >> 6, l = i & 63;
    int row = row0 + (l & 31);
    row = row < nb ? row : nb - 1;
    const float* p = x + (int64_t)row * ldx + 16 * ks + 8 * (l >> 5);
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
    uint32_t h4[4], l4[4];
    split2(a[0], a[1], h4[0], l4[0]);
    split2(a[2], a[3], h4[1], l4[1]);
    split2(b[0], b[1], h4[2], l4[2]);
    split2(b[2], b[3], h4[3], l4[3]);
    *(uint4*)(smem + (size_t)(2 * ks) * 1024 + l * 16) = make_uint4(h4[0], h4[1], h4[2], h4[3]);
    *(uint4*)(smem + (size_t)(2 * ks + 1) * 1024 + l * 16) = make_uint4(l4[0], l4[1], l4[2], l4[3]);
  }

  const int j = slab * tiles + wave;  // the wave's hidden tile: units 32 j .. 32 j + 31
  const uint16_t* w1p = img + (int64_t)j * ks1 * 1024 + lane * 8;
  const uint16_t* w2p = img + (int64_t)8 * d * d + (int64_t)j * 2 * NU * 1024 + lane * 8;

  bf16x8 wa[4][2], wb[4][2];
  auto ldw = [&](bf16x8(&w)[4][2], int ks0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      w[q][0] = *(const bf16x8*)(w1p + (int64_t)(ks0 + q) * 1024);
      w[q][1] = *(const bf16x8*)(w1p + (int64_t)(ks0 + q) * 1024 + 512);
    }
  };
  ldw(wa, 0);
  // C <= 64: fc2's 8 W2 fragments travel beside fc1
  constexpr bool W2_EARLY = NU <= 2;
  bf16x8 w2f[2][NU][2];
  auto ldw2 = [&]() {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        w2f[s2][u][0] = *(const bf16x8*)(w2p + (s2 * NU + u) * 1024);
        w2f[s2][u][1] = *(const bf16x8*)(w2p + (s2 * NU + u) * 1024 + 512);
      }
  };
  if constexpr (W2_EARLY) ldw2();

  // fc1: two accumulators (even / odd k-steps), the first starting at the bias
  // (lane: hidden 32 j + 8 i + 4 hf + rr of query row r)
  f32x16 a0, a1 = (f32x16){0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 bb = *(const f32x4*)(b1 + 32 * j + 8 * i + 4 * hf);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) a0[4 * i + rr] = bb[rr];
  }
  __syncthreads();  // the x images are complete
  auto mac4 = [&](const bf16x8(&w)[4][2], int ks0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bf16x8 xh = *(const bf16x8*)(smem + (size_t)(2 * (ks0 + q)) * 1024 + lane * 16);
      const bf16x8 xl = *(const bf16x8*)(smem + (size_t)(2 * (ks0 + q) + 1) * 1024 + lane * 16);
      if (q & 1) {
        a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[q][0], xh, a1, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[q][0], xl, a1, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[q][1], xh, a1, 0, 0, 0);
      } else {
        a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[q][0], xh, a0, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[q][0], xl, a0, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[q][1], xh, a0, 0, 0, 0);
      }
    }
  };
  for (int ks0 = 0; ks0 < ks1; ks0 += 8) {  // ks1 % 8 == 0 (D % 128 == 0)
    ldw(wb, ks0 + 4);
    mac4(wa, ks0);
    if (ks0 + 8 < ks1) ldw(wa, ks0 + 8);
    mac4(wb, ks0 + 4);
  }
  if constexpr (!W2_EARLY) ldw2();

  // GELU, split into fc2's B operands (k-step s2: hidden 32 j + 16 s2 + 8 (e >> 2) + 4 hf + (e & 3))
  uint32_t hph[8], hpl[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    split2(mmr::gelu_erf(a0[4 * i] + a1[4 * i]), mmr::gelu_erf(a0[4 * i + 1] + a1[4 * i + 1]), hph[2 * i], hpl[2 * i]);
    split2(mmr::gelu_erf(a0[4 * i + 2] + a1[4 * i + 2]), mmr::gelu_erf(a0[4 * i + 3] + a1[4 * i + 3]), hph[2 * i + 1],
           hpl[2 * i + 1]);
  }
  f32x16 acc2[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) acc2[u] = (f32x16){0};
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const bf16x8 hfh = __builtin_bit_cast(bf16x8, make_uint4(hph[4 * s2], hph[4 * s2 + 1], hph[4 * s2 + 2],
                                                             hph[4 * s2 + 3]));
    const bf16x8 hfl = __builtin_bit_cast(bf16x8, make_uint4(hpl[4 * s2], hpl[4 * s2 + 1], hpl[4 * s2 + 2],
                                                             hpl[4 * s2 + 3]));
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      acc2[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[s2][u][0], hfh, acc2[u], 0, 0, 0);
      acc2[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[s2][u][0], hfl, acc2[u], 0, 0, 0);
      acc2[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2f[s2][u][1], hfh, acc2[u], 0, 0, 0);
    }
  }

  // the waves' [32 classes][32 rows] tiles summed in wave order through LDS (red[wave][row][33]), one
  // 32-class slice at a time; lane holds classes 32 u + 8 i + 4 hf + rr of row r
  __syncthreads();  // every wave is done with the x images
  float* red = (float*)smem;
  const int nu = cp / 32;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    if (u < nu) {  // uniform
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) red[(wave * 32 + r) * 33 + 8 * i + 4 * hf + rr] = acc2[u][4 * i + rr];
      __syncthreads();
      for (int e = threadIdx.x; e < 1024; e += nthr) {
        const int row = e >> 5, col = e & 31;
        float v = red[row * 33 + col];
        for (int w = 1; w < tiles; ++w) v += red[(w * 32 + row) * 33 + col];
        if (row0 + row < nb) work[((int64_t)slab * nb + row0 + row) * cp + 32 * u + col] = v;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(256) void cls_head_finish(const float* __restrict__ work, int ns,
                                                       const float* __restrict__ b2, float* __restrict__ logits,
                                                       float* __restrict__ probs, int32_t* __restrict__ preds,
                                                       float* __restrict__ topk_vals, int32_t* __restrict__ topk_idx,
                                                       int nb, int c, int cp, int k, float thr) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= nb) return;
  float p[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int cc = lane + 64 * q;
    p[q] = -1.0f;  // below every probability: classes >= C never count
    if (cc < c) {
      float v = work[row * cp + cc];
      for (int s = 1; s < ns; ++s) v += work[((int64_t)s * nb + row) * cp + cc];
      v += b2[cc];
      logits[row * c + cc] = v;
      // 1 / (1 + e^-v); the exponent stops at 88 (e^88 < FLT_MAX: a logit below -88 gives ~6e-39, not 1 / inf)
      const float pr = __fdiv_rn(1.0f, 1.0f + mmr::exp_acc(fminf(-v, 88.0f)));
      p[q] = pr;
      if (probs) probs[row * c + cc] = pr;
      if (preds) preds[row * c + cc] = pr >= thr ? 1 : 0;
    }
  }
  if (!topk_vals && !topk_idx) return;
  // rank of class cc = the number of classes ahead of it in (prob desc, class asc): a permutation of 0 .. C - 1
  int rank[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q2 = 0; q2 < 4; ++q2) {
    const int n = c - 64 * q2 < 64 ? c - 64 * q2 : 64;
    for (int l2 = 0; l2 < n; ++l2) {  // uniform
      const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p[q2]), l2));
      const int c2 = 64 * q2 + l2;
#pragma unroll
      for (int q = 0; q < 4; ++q) rank[q] += (v > p[q] || (v == p[q] && c2 < lane + 64 * q)) ? 1 : 0;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int cc = lane + 64 * q;
    if (cc < c && rank[q] < k) {
      if (topk_vals) topk_vals[row * k + rank[q]] = p[q];
      if (topk_idx) topk_idx[row * k + rank[q]] = cc;
    }
  }
}

template <int NU>
void launch_partial(const float* x, int64_t ldx, const uint16_t* img, const float* b1, float* work, int b, int d, int cp,
                    hipStream_t st) {
  const int tiles = cls_slab_tiles(d);
  const size_t red = (size_t)tiles * 32 * 33 * 4, xi = (size_t)d * 128;
  const dim3 grid((unsigned)mmr::ceil_div(b, 32), (unsigned)cls_slabs(d));
  cls_head_partial<NU><<<grid, 64 * tiles, xi > red ? xi : red, st>>>(x, ldx, img, b1, work, b, d, cp, tiles);
}

}  // namespace

extern "C" {

int64_t mmr_classifier_pack_bytes(int32_t d, int32_t h, int32_t c) {
  const int64_t cp = cls_cp(c);
  switch (cls_route(d, h, c)) {
    case CLS_FUSED: return ((int64_t)h * d * 2 + (int64_t)h * cls_nut(c) * 64) * 2;
    case CLS_CHAIN_X3: return ((int64_t)h * d + cp * h) * 4;
    case CLS_CHAIN_F32: return ((int64_t)h * d + cp * h) * 4;
    default: return 0;
  }
}

mmr_status mmr_classifier_pack(const float* w1, const float* w2, void* images, int32_t d, int32_t h, int32_t c,
                               void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(w1 && w2 && images, "mmr_classifier_pack: NULL pointer");
  MMR_REQUIRE(d > 0 && h > 0 && c >= 1, "mmr_classifier_pack: d=%d h=%d c=%d", d, h, c);
  MMR_REQUIRE(aligned16(images), "mmr_classifier_pack: images must be 16-B aligned");
  const int route = cls_route(d, h, c);
  if (route == CLS_NONE) {
    mmr::set_error("mmr_classifier_pack: d=%d h=%d c=%d not built (c <= %d; d %% 16 == 0, h %% 32 == 0)", d, h, c,
                   CLS_MAX_C);
    return MMR_ERR_UNSUPPORTED;
  }
  hipStream_t st = mmr::as_stream(stream);
  const int cp = cls_cp(c);
  if (route == CLS_FUSED) {
    const int nut = cls_nut(c);
    const int64_t n = (int64_t)h * d * 2 + (int64_t)h * nut * 64;
    cls_pack_fused<<<dim3((unsigned)mmr::ceil_div(n, 256)), 256, 0, st>>>(w1, w2, (uint16_t*)images, d, h, c, nut);
  } else {
    const int64_t n = (int64_t)h * d + (int64_t)cp * h;
    const dim3 grid((unsigned)mmr::ceil_div(n, 256));
    if (route == CLS_CHAIN_X3) cls_pack_chain<true><<<grid, 256, 0, st>>>(w1, w2, images, d, h, c, cp);
    else cls_pack_chain<false><<<grid, 256, 0, st>>>(w1, w2, images, d, h, c, cp);
  }
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

int64_t mmr_classifier_work_bytes(int32_t b, int32_t d, int32_t h, int32_t c) {
  if (b < 0) return 0;
  const int cp = cls_cp(c);
  switch (cls_route(d, h, c)) {
    case CLS_FUSED: return (int64_t)cls_slabs(d) * b * cp * 4;
    case CLS_CHAIN_X3:
    case CLS_CHAIN_F32: return cls_part_bytes(b, cp) + (int64_t)b * h * 4;
    default: return 0;
  }
}

mmr_status mmr_classifier_head(const float* x, int64_t ldx, const void* images, const float* b1, const float* b2,
                               void* work, float* logits, float* probs, int32_t* preds, float* topk_vals,
                               int32_t* topk_idx, int32_t b, int32_t d, int32_t h, int32_t c, int32_t k,
                               float threshold, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(x && logits, "mmr_classifier_head: NULL x or logits");
  MMR_REQUIRE(images && b1 && b2 && work, "mmr_classifier_head: NULL images / b1 / b2 / work");
  MMR_REQUIRE(c >= 1, "mmr_classifier_head: c=%d < 1", c);
  MMR_REQUIRE(b >= 0 && d > 0 && h > 0, "mmr_classifier_head: b=%d d=%d h=%d", b, d, h);
  const bool topk = topk_vals || topk_idx;
  MMR_REQUIRE(!topk || (k >= 1 && k <= c), "mmr_classifier_head: k=%d outside 1..c=%d", k, c);
  const int route = cls_route(d, h, c);
  if (route == CLS_NONE) {
    mmr::set_error("mmr_classifier_head: d=%d h=%d c=%d not built (c <= %d; d %% 16 == 0, h %% 32 == 0)", d, h, c,
                   CLS_MAX_C);
    return MMR_ERR_UNSUPPORTED;
  }
  MMR_REQUIRE(ldx >= d && ldx % 4 == 0, "mmr_classifier_head: ldx=%lld (>= d, %% 4 == 0)", (long long)ldx);
  MMR_REQUIRE(aligned16(x) && aligned16(images) && aligned16(b1) && aligned16(work),
              "mmr_classifier_head: x / images / b1 / work 16-B aligned");
  if (b == 0) return MMR_OK;
  hipStream_t st = mmr::as_stream(stream);
  const int cp = cls_cp(c);
  int ns = 1;
  if (route == CLS_FUSED) {
    ns = cls_slabs(d);
    const uint16_t* img = (const uint16_t*)images;
    const int nut = cls_nut(c);
    if (nut == 2) launch_partial<2>(x, ldx, img, b1, (float*)work, b, d, cp, st);
    else if (nut == 4) launch_partial<4>(x, ldx, img, b1, (float*)work, b, d, cp, st);
    else launch_partial<8>(x, ldx, img, b1, (float*)work, b, d, cp, st);
    MMR_LAUNCH_CHECK();
  } else {
    float* part = (float*)work;
    float* hid = (float*)((char*)work + cls_part_bytes(b, cp));
    const int64_t n1 = (int64_t)h * d, n2 = (int64_t)cp * h;
    mmr_status s;
    if (route == CLS_CHAIN_X3) {
      const uint16_t* o = (const uint16_t*)images;
      s = mmr_linear_x3(x, ldx, 0, o, o + n1, 0, b1, 0, nullptr, 0, 0, hid, h, 0, 1, b, d, h, 1, stream);
      if (s != MMR_OK) return s;
      s = mmr_linear_x3(hid, h, 0, o + 2 * n1, o + 2 * n1 + n2, 0, nullptr, 0, nullptr, 0, 0, part, cp, 0, 1, b, h, cp,
                        0, stream);
    } else {
      const float* o = (const float*)images;
      s = mmr_linear_f32(x, ldx, o, b1, nullptr, 0, hid, h, b, d, h, 1, stream);
      if (s != MMR_OK) return s;
      s = mmr_linear_f32(hid, h, o + n1, nullptr, nullptr, 0, part, cp, b, h, cp, 0, stream);
    }
    if (s != MMR_OK) return s;
  }
  cls_head_finish<<<dim3((unsigned)mmr::ceil_div(b, 4)), 256, 0, st>>>((const float*)work, ns, b2, logits, probs, preds,
                                                                      topk_vals, topk_idx, b, c, cp, k, threshold);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

}  // extern "C"
