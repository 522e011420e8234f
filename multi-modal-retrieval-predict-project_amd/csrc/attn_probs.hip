// Head-averaged attention probabilities: what nn.MultiheadAttention returns beside its output with its
// defaults (need_weights = True, average_attn_weights = True), eval, no masks —
//   P[b][r][c] = (1 / H) sum_h softmax_c(q_h[b][r] . k_h[b][c] * scale)
// the reference's `attn` maps (src/Model/fusion.py:427,433 txt2img / img2txt, model.py:399 comb).  The
// attention cores (fusion.hip mha_small, x3.hip x3_mha) keep the softmax in registers and never hold P,
// so the maps are a kernel of their own, launched only when a caller asks for them.
//
// One wave owns a 32-query tile of one batch element and loops over the heads itself (no atomics, a fixed
// head order: two launches give the same bits).  S^T = K . Q^T on v_mfma_f32_32x32x16_bf16, x3_mha's
// layout: the query sits on the lane, so the row max / sum stay in registers.  bf16 rows: one product per
// q.k (bf16 x bf16 is exact in f32).  f32 rows (x3): q and k split hi / lo in registers, Kh.Qh + Kh.Ql +
// Kl.Qh as x3_mha.  The MFMA's K operand of lane (key r, half hf) is 8 consecutive d of key row r: a 16-B
// (bf16) or 2 x 16-B (f32) global load straight into the fragment, so nothing is staged in LDS and the
// waves of a block never synchronise (the K rows of a batch element are re-read from L2 by its few
// query tiles; the maps are 4 lq lk bytes per batch element against 2-4 lk heads dh of K).
//   pass A  per head: online (max, sum) over 32-key tiles -> (m_h, 1 / l_h) per query, kept in LDS
//           ([heads][32] per wave: a register array indexed by a runtime head count would live in scratch);
//   pass B  per 64-key block, per head: the same score tile by the same instruction sequence (the scaled
//           score is rounded on its own, mmr::mul_rn, so neither pass contracts it into the subtraction:
//           exp(s - m_h) is pass A's, bit for bit), acc += exp(s - m_h) / l_h; acc / heads goes through a
//           wave-private LDS tile so that each global store instruction writes one row's <= 64 consecutive
//           floats (lane = column: coalesced at any ldp / alignment, never past column lk).
#include <math.h>

#include <algorithm>

#include "common.h"

namespace {

using mmr::aligned16;
using mmr::bf16x8;
using mmr::f32x16;
using mmr::LGKM0;

constexpr int AP_KB = 64;           // keys per pass-B block: two 32-key MFMA tiles
constexpr int AP_TROW = AP_KB + 1;  // floats per row of the transpose tile (odd: the column writes spread over banks)
constexpr size_t AP_LDS_MAX = 64 * 1024;

struct ProbArgs {
  const void* q;
  int64_t ldq;
  const void* k;
  int64_t ldk;
  float* probs;
  int64_t ldp;
  int lq, lk, heads, dh;
  float scale, inv_heads;
  int nqt;        // 32-query tiles per batch element
  int64_t units;  // b * nqt, one per wave
};

constexpr size_t ap_wave_lds(int heads) { return (size_t)heads * 32 * 8 + (size_t)32 * AP_TROW * 4; }

// f32 x8 -> (hi, lo) bf16 x8: mmr::split8's arithmetic with all four hi words formed first.  Kept apart from it:
// on mmr::split8 attn_probs<2, true> goes from 178 to 148 VGPRs (tools/isa_diff.py), 2 -> 3 waves per SIMD, and
// no timer reaches these kernels to say what that does to them
__device__ __forceinline__ void split8(const float4 a, const float4 b, bf16x8& hi, bf16x8& lo) {
  const uint32_t h0 = mmr::pack2bf(a.x, a.y), h1 = mmr::pack2bf(a.z, a.w);
  const uint32_t h2 = mmr::pack2bf(b.x, b.y), h3 = mmr::pack2bf(b.z, b.w);
  const uint32_t l0 = mmr::pack2bf(a.x - __uint_as_float(h0 << 16), a.y - __uint_as_float(h0 & 0xFFFF0000u));
  const uint32_t l1 = mmr::pack2bf(a.z - __uint_as_float(h1 << 16), a.w - __uint_as_float(h1 & 0xFFFF0000u));
  const uint32_t l2 = mmr::pack2bf(b.x - __uint_as_float(h2 << 16), b.y - __uint_as_float(h2 & 0xFFFF0000u));
  const uint32_t l3 = mmr::pack2bf(b.z - __uint_as_float(h3 << 16), b.w - __uint_as_float(h3 & 0xFFFF0000u));
  hi = __builtin_bit_cast(bf16x8, make_uint4(h0, h1, h2, h3));
  lo = __builtin_bit_cast(bf16x8, make_uint4(l0, l1, l2, l3));
}

// The MFMA fragments of one row (element offset `row` = its head's first column): lane half hf holds
// d = 16 ks + 8 hf .. + 7 of K-step ks; chunks at d >= dh read the row's first chunk (in bounds) and are zeroed
template <int KS, bool X3>
struct RowFrag {
  bf16x8 hi[KS], lo[X3 ? KS : 1];
  __device__ __forceinline__ void load(const void* base, int64_t row, int dh, int hf) {
    if constexpr (X3) {
      float4 x[KS][2];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int d = 16 * ks + 8 * hf;
        const float* p = (const float*)base + row + (d < dh ? d : 0);
        x[ks][0] = *(const float4*)p;
        x[ks][1] = *(const float4*)(p + 4);
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (16 * ks + 8 * hf >= dh) x[ks][0] = x[ks][1] = make_float4(0.f, 0.f, 0.f, 0.f);
        split8(x[ks][0], x[ks][1], hi[ks], lo[ks]);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int d = 16 * ks + 8 * hf;
        uint4 v = *(const uint4*)((const uint16_t*)base + row + (d < dh ? d : 0));
        if (d >= dh) v = make_uint4(0u, 0u, 0u, 0u);
        hi[ks] = __builtin_bit_cast(bf16x8, v);
      }
    }
  }
};

// Scaled scores of 32 keys from k0 against the wave's 32 queries: lane (query r, half hf), register rg =
// key k0 + (rg & 3) + 8 (rg >> 2) + 4 hf; keys >= lk are -inf (their K rows read key lk - 1).  Both passes
// call this, so a score has the same bits in both.
template <int KS, bool X3>
__device__ __forceinline__ f32x16 score_tile(const ProbArgs& a, int64_t kbase, int k0, int r, int hf,
                                             const RowFrag<KS, X3>& qf) {
  const int key = k0 + r < a.lk ? k0 + r : a.lk - 1;
  RowFrag<KS, X3> kf;
  kf.load(a.k, kbase + (int64_t)key * a.ldk, a.dh, hf);
  f32x16 s = (f32x16){0};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.hi[ks], qf.hi[ks], s, 0, 0, 0);
    if constexpr (X3) {
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.hi[ks], qf.lo[ks], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf.lo[ks], qf.hi[ks], s, 0, 0, 0);
    }
  }
#pragma unroll
  for (int rg = 0; rg < 16; ++rg) {
    const int kk = k0 + (rg & 3) + 8 * (rg >> 2) + 4 * hf;
    s[rg] = kk < a.lk ? mmr::mul_rn(s[rg], a.scale) : -INFINITY;
  }
  return s;
}

// this wave's LDS writes landed and visible to its other lanes (the LDS regions are wave-private)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_s_waitcnt(LGKM0);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
}

template <int DT, bool X3>
__global__ __launch_bounds__(256) void attn_probs(const ProbArgs a) {
  constexpr int KS = 2 * DT;  // K-steps of 16 over the head dim padded to 32 DT
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  const int64_t unit = (int64_t)blockIdx.x * nwv + wave;
  if (unit >= a.units) return;  // wave-uniform; the waves of a block share nothing
  const int64_t bi = unit / a.nqt;
  const int q0 = (int)(unit - bi * a.nqt) * 32;
  const int r = lane & 31, hf = lane >> 5;
  const int lq = a.lq, lk = a.lk, heads = a.heads, dh = a.dh;
  float2* ml = (float2*)(smem + (size_t)wave * ap_wave_lds(heads));  // [heads][32]: (m_h, 1 / l_h) per query
  float* tile = (float*)(ml + heads * 32);                           // [32][AP_TROW]
  const int qi = q0 + r < lq ? q0 + r : lq - 1;  // queries past lq: computed from row lq - 1, never stored
  const int64_t qrow = (bi * lq + qi) * a.ldq, krow0 = bi * lk * a.ldk;

  // pass A
  for (int h = 0; h < heads; ++h) {
    RowFrag<KS, X3> qf;
    qf.load(a.q, qrow + h * dh, dh, hf);
    float m_run = -INFINITY, l_run = 0.f;
    for (int k0 = 0; k0 < lk; k0 += 32) {
      const f32x16 s = score_tile<KS, X3>(a, krow0 + h * dh, k0, r, hf, qf);
      float mloc = s[0];
#pragma unroll
      for (int rg = 1; rg < 16; ++rg) mloc = fmaxf(mloc, s[rg]);
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));  // finite: key k0 < lk is in the tile
      const float m_new = fmaxf(m_run, mloc);
      const float alpha = m_run == -INFINITY ? 0.f : mmr::exp_acc(m_run - m_new);
      float psum = 0.f;
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) psum += s[rg] == -INFINITY ? 0.f : mmr::exp_acc(s[rg] - m_new);
      l_run = l_run * alpha + psum;
      m_run = m_new;
    }
    l_run += __shfl_xor(l_run, 32, 64);
    if (hf == 0) ml[h * 32 + r] = make_float2(m_run, 1.0f / l_run);
  }
  wave_lds_sync();

  // pass B
  for (int k0 = 0; k0 < lk; k0 += AP_KB) {
    const bool two = k0 + 32 < lk;  // wave-uniform: the block's second tile holds a key
    f32x16 acc[2] = {(f32x16){0}, (f32x16){0}};
    for (int h = 0; h < heads; ++h) {
      RowFrag<KS, X3> qf;
      qf.load(a.q, qrow + h * dh, dh, hf);
      const float2 mi = ml[h * 32 + r];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t == 1 && !two) continue;
        const f32x16 s = score_tile<KS, X3>(a, krow0 + h * dh, k0 + 32 * t, r, hf, qf);
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) acc[t][rg] += s[rg] == -INFINITY ? 0.f : mmr::exp_acc(s[rg] - mi.x) * mi.y;
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg)
        tile[r * AP_TROW + 32 * t + (rg & 3) + 8 * (rg >> 2) + 4 * hf] = acc[t][rg] * a.inv_heads;
    wave_lds_sync();
    const int nk = lk - k0 < AP_KB ? lk - k0 : AP_KB;
    const int nrow = lq - q0 < 32 ? lq - q0 : 32;
    float* dst = a.probs + (bi * lq + q0) * a.ldp + k0 + lane;
    if (lane < nk)
      for (int row = 0; row < nrow; ++row) dst[row * a.ldp] = tile[row * AP_TROW + lane];
    wave_lds_sync();  // the tile is read before the next block overwrites it
  }
}

template <bool X3>
mmr_status launch_probs(const char* who, const void* q, int64_t ldq, const void* k, int64_t ldk, float* probs,
                        int64_t ldp, int32_t b, int32_t lq, int32_t lk, int32_t heads, int32_t dh, float scale,
                        void* stream) {
  constexpr int MAXDH = X3 ? 128 : 192, AL = X3 ? 4 : 8;
  MMR_REQUIRE(q && k && probs, "%s: NULL pointer", who);
  MMR_REQUIRE(b >= 0 && lq > 0 && lk > 0 && heads > 0 && dh > 0 && dh % 8 == 0 && dh <= MAXDH,
              "%s: bad shape b=%d lq=%d lk=%d heads=%d head_dim %d (head_dim %% 8 == 0, <= %d)", who, b, lq, lk, heads,
              dh, MAXDH);
  MMR_REQUIRE(ldq % AL == 0 && ldk % AL == 0 && aligned16(q) && aligned16(k) && (int64_t)heads * dh <= ldq &&
                  (int64_t)heads * dh <= ldk,
              "%s: q / k rows must be 16-B aligned with strides >= heads*dh", who);
  MMR_REQUIRE(ldp >= lk && ((uintptr_t)probs & 3u) == 0, "%s: ldp=%lld below lk=%d (or probs misaligned)", who,
              (long long)ldp, lk);
  if (b == 0) return MMR_OK;
  // waves per block: as many of 4 as the per-wave (m, 1 / l) tables leave room for
  int wpb = 4;
  while (wpb > 1 && wpb * ap_wave_lds(heads) > AP_LDS_MAX) wpb >>= 1;
  if (ap_wave_lds(heads) > AP_LDS_MAX) {
    mmr::set_error("%s: heads=%d: the per-head softmax statistics do not fit in LDS (heads <= %d)", who, heads,
                   (int)((AP_LDS_MAX - 32 * AP_TROW * 4) / 256));
    return MMR_ERR_UNSUPPORTED;
  }
  ProbArgs a{q, ldq, k, ldk, probs, ldp, lq, lk, heads, dh, scale, 1.0f / (float)heads, (lq + 31) / 32, 0};
  a.units = (int64_t)b * a.nqt;
  const int64_t nblk = mmr::ceil_div(a.units, wpb);
  MMR_REQUIRE(nblk < (int64_t(1) << 31), "%s: too many query tiles", who);
  const dim3 grid((unsigned)nblk), blk(64 * wpb);
  const size_t lds = wpb * ap_wave_lds(heads);
  hipStream_t st = mmr::as_stream(stream);
  switch ((dh + 31) / 32) {
    case 1: attn_probs<1, X3><<<grid, blk, lds, st>>>(a); break;
    case 2: attn_probs<2, X3><<<grid, blk, lds, st>>>(a); break;
    case 3: attn_probs<3, X3><<<grid, blk, lds, st>>>(a); break;
    case 4: attn_probs<4, X3><<<grid, blk, lds, st>>>(a); break;
    case 5:
      if constexpr (!X3) attn_probs<5, false><<<grid, blk, lds, st>>>(a);
      break;
    default:
      if constexpr (!X3) attn_probs<6, false><<<grid, blk, lds, st>>>(a);
      break;
  }
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

}  // namespace

extern "C" {

mmr_status mmr_mha_probs(const uint16_t* q, int64_t ldq, const uint16_t* k, int64_t ldk, float* probs, int64_t ldp,
                         int32_t b, int32_t lq, int32_t lk, int32_t heads, int32_t dh, float scale, void* stream) {
  mmr::clear_error();
  return launch_probs<false>("mmr_mha_probs", q, ldq, k, ldk, probs, ldp, b, lq, lk, heads, dh, scale, stream);
}

mmr_status mmr_x3_attention_probs(const float* q, int64_t ldq, const float* k, int64_t ldk, float* probs, int64_t ldp,
                                  int32_t b, int32_t lq, int32_t lk, int32_t heads, int32_t dh, float scale,
                                  void* stream) {
  mmr::clear_error();
  return launch_probs<true>("mmr_x3_attention_probs", q, ldq, k, ldk, probs, ldp, b, lq, lk, heads, dh, scale,
                            stream);
}

}  // extern "C"
