// Streaming route of mmr_swin_window_attention (7 x 7 windows, an even number of 32-wide heads).
//
// The arithmetic is tower.hip's swin_window_attention<false>, operation for operation (same
// fragment-to-lane mapping, S accumulators started from bias * sqrt(dh), four-chain max / sum, the
// same exp2 form, packing and 1 / psum), so the output is bit-identical; what changes is how the
// bytes move (the gather kernel keeps the texture addresser 61-86 % busy at 2.8-3.4 TB/s with MFMA
// under 5 %: profiles/r07_swa_pmc.txt):
//   * a unit is (image, window, HEAD PAIR); its 49 token rows' q | k | v segments of the pair (3 x 128 B
//     per token: whole cache lines, used by the wave that fetched them) are gathered through the
//     cyclic shift into a per-wave LDS image by LDS-DMA: 20 wave instructions of 1 KiB, 8 lanes per
//     128-B segment, instead of 24 fragment-shaped loads that touch 32 token rows each;
//   * the image row is 25 16-B chunks (24 + 1 pad, the pad chunk re-reads the row's first chunk): a
//     400-B stride puts 16 consecutive tokens on disjoint bank quads, so the Q / K fragments are
//     conflict-free ds_read_b128; V^T fragments come by ds_read_b64_tr_b16 from the same image.
//     Lanes of padded tokens (>= 49) read row 0, as the gather kernel's clamped loads do;
//   * O is staged over the pair's (consumed) Q bytes and leaves as 16-B chunks, 8 lanes per 128-B
//     output segment, through the reverse roll: 7 store instructions per pair instead of 16;
//   * the dense bias rows (32 of the gather kernel's 56 load instructions per head pair, each touching
//     32 rows of an L2-resident tile) depend on (window type, head pair) only.  Units are ordered
//     (window, head pair)-major with the images innermost and every wave takes one contiguous range of
//     that order, so a wave keeps its lanes' rows in registers, already multiplied by sqrt(dh) (the
//     same rounded product the gather kernel forms per unit), and re-reads them only where its range
//     crosses into the next (window, head pair);
//   * one persistent workgroup of 4 waves per CU, two images per wave.  Per unit: wait for this unit's
//     image (issued one unit ago), store the previous unit's staged output, read every MFMA operand of
//     the unit out of LDS, issue the next unit's gather into the buffer the stored output left, then
//     compute from registers.  hipcc makes every LDS access it knows of, and every use of a plain
//     load's result, wait for all LDS-DMA in flight (vmcnt(0)): hence the operand reads before the
//     gather, the output staging through an inline-asm ds_write, and no plain load in that span.
// Forms measured and dropped (profiles/r07_swa_stream_ab.txt): the bias rows re-read per unit with 8
// waves and one image each, or with 4 waves, two images and a second register set for the next unit's
// rows.
#include <float.h>

#include <algorithm>

#include "common.h"

namespace {

using mmr::bf16x4;
using mmr::bf16x8;
using mmr::f32x16;
using mmr::LGKM0;
using mmr::u32x2;
using mmr::vmcnt_n;
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int SWS = 7, STOK = 49;
constexpr int NW = mmr::SWA_STREAM_WAVES;
constexpr int ROWCH = 25;               // 16-B chunks per image row: q pair 8 | k pair 8 | v pair 8 | pad
constexpr int ROW_B = ROWCH * 16;       // 400 B
constexpr int NDMA = 20;                // LDS-DMA instructions per image (49 x 25 = 1225 chunks of 1280)
constexpr int IMG_B = NDMA * 1024;
constexpr int LDS_B = NW * 2 * IMG_B;
constexpr int OCH = STOK * 8;           // 16-B output chunks per unit
constexpr int NOST = (OCH + 63) / 64;   // output store instructions per unit
static_assert(STOK * ROWCH <= NDMA * 64, "image chunks");
static_assert(LDS_B <= 160 * 1024, "LDS budget");

// 8-B LDS write the compiler does not see as one (see the header): LDS operations of a wave execute
// in order, so the later reads of these bytes (ordinary loads, after an lgkmcnt(0)) see them.
__device__ __forceinline__ void lds_write_b64(unsigned char* p, uint32_t lo, uint32_t hi) {
  const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)p;
  const u32x2 v = {lo, hi};
  asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(v) : "memory");
}

struct Unit {  // wave-uniform
  uint32_t tok0;  // first token of the image
  int hs, ws_, type, hp;
  int combo;  // window * head pairs + hp: what the bias rows depend on
};
struct Frags {  // a head's MFMA operands
  bf16x8 qf[2][2], kf[2][2], vf[2][2];
};

__global__ __launch_bounds__(NW * 64) void swin_wattn_stream(const uint16_t* __restrict__ qkv,
                                                             const float* __restrict__ bias,
                                                             uint16_t* __restrict__ out, int units, int nimg,
                                                             int H, int C, int heads, int shift) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  unsigned char* img0 = smem + wave * (2 * IMG_B);
  const int nw1 = H / SWS, npair = heads >> 1;
  // wave g of G takes the units [g U / G, (g + 1) U / G) of the (window, head pair)-major order
  const int64_t G = (int64_t)gridDim.x * NW, g = blockIdx.x * NW + wave;
  const int i0 = (int)(g * units / G), i1 = (int)((g + 1) * units / G);
  if (i0 >= i1) return;  // no workgroup barrier anywhere below

  // per-lane gather coordinates, fixed for the launch: image chunk p = 64 it + lane holds token
  // p / 25, 16-B unit p % 25 (the pad unit and the tail past token 48 re-read token 0's unit 0);
  // packed ty | tx << 4 | (column offset inside the token's qkv row, without the pair's) << 8
  uint32_t gc[NDMA];
#pragma unroll
  for (int it = 0; it < NDMA; ++it) {
    const int p = it * 64 + lane;
    int t = p / ROWCH, un = p - t * ROWCH;
    if (un == ROWCH - 1 || t >= STOK) t = 0, un = 0;
    gc[it] = (uint32_t)(t / SWS) | ((uint32_t)(t % SWS) << 4) | ((uint32_t)((un >> 3) * C + (un & 7) * 8) << 8);
  }
  // rolled window coordinate -> token row inside the image (wrap as an unsigned min)
  auto img_row = [&](int hs, int ws_, int ty, int tx) -> uint32_t {
    uint32_t hh = (uint32_t)(hs + ty), ww = (uint32_t)(ws_ + tx);
    hh = min(hh, hh - (uint32_t)H);
    ww = min(ww, ww - (uint32_t)H);
    return hh * (uint32_t)H + ww;
  };
  auto unit_of = [&](int i) -> Unit {  // unit i = combo * nimg + image; pinned to SGPRs
    const int combo = __builtin_amdgcn_readfirstlane(i / nimg), bi = i - combo * nimg;
    const int wi = __builtin_amdgcn_readfirstlane(combo / npair);
    const int wy = __builtin_amdgcn_readfirstlane(wi / nw1), wx = wi - wy * nw1;
    Unit o;
    o.combo = combo;
    o.hp = combo - wi * npair;
    o.tok0 = (uint32_t)bi * (uint32_t)(H * H);
    o.hs = wy * SWS + shift;
    o.ws_ = wx * SWS + shift;
    o.type = shift > 0 ? ((wy == nw1 - 1) ? 2 : 0) + ((wx == nw1 - 1) ? 1 : 0) : 0;
    return o;
  };
  const uint32_t rs = 3u * (uint32_t)C;  // element offsets fit 32 bits (launcher)
  auto gather = [&](const Unit& un, unsigned char* dst) {
#pragma unroll
    for (int it = 0; it < NDMA; ++it) {
      const uint32_t c = gc[it];
      const uint32_t row = img_row(un.hs, un.ws_, (int)(c & 15u), (int)((c >> 4) & 15u));
      const uint16_t* src = qkv + ((un.tok0 + row) * rs + (c >> 8) + (uint32_t)(un.hp * 64));
      __builtin_amdgcn_global_load_lds((const void*)src, (lds_ptr_t)(dst + it * 1024), 16, 0, 0);
    }
  };

  const int r = lane & 31, hf = lane >> 5;
  const int grp = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  constexpr float L2E = 1.4426950408889634f;
  const float scale = 0.17677669529663687f;  // 32^-0.5
  const float rscale = 5.656854249492381f;     // 32^0.5

  // bias rows of this lane's two queries of head 2 hp + h2 ([qt][kt]; element 4 g4 + e = key
  // kt 32 + 8 g4 + 4 hf + e) as bias / scale (-FLT_MAX padding -> -inf: exp2 -> 0)
  auto load_bias = [&](f32x16 (&sa)[2][2], const Unit& un, int h2) {
    const float* bt = bias + ((int64_t)un.type * heads + (2 * un.hp + h2)) * 4096;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const float4 bv = *(const float4*)(bt + (qt * 32 + r) * 64 + kt * 32 + 8 * g4 + 4 * hf);
          sa[qt][kt][4 * g4] = bv.x;
          sa[qt][kt][4 * g4 + 1] = bv.y;
          sa[qt][kt][4 * g4 + 2] = bv.z;
          sa[qt][kt][4 * g4 + 3] = bv.w;
        }
        sa[qt][kt] *= rscale;
      }
  };
  // Q / K fragments (token t2 32 + r, dims 16 ks + 8 hf ..) and the V^T fragments (lane: dim r,
  // keys in P^T's register order) by ds_read_b64_tr_b16 pairs from the key-major V segment
  auto read_frags = [&](const unsigned char* im, int h2, Frags& f) {
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      const int t = t2 * 32 + r;
      const unsigned char* row = im + (t < STOK ? t : 0) * ROW_B + h2 * 64 + 16 * hf;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        f.qf[t2][ks] = *(const bf16x8*)(row + ks * 32);
        f.kf[t2][ks] = *(const bf16x8*)(row + 128 + ks * 32);
      }
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int sidx = 0; sidx < 2; ++sidx) {
        const int k0 = kt * 32 + 16 * sidx + 4 * (grp >> 1) + tq, k1 = k0 + 8;
        const int voff = 256 + h2 * 64 + ((grp & 1) * 16 + 4 * tp) * 2;
        const unsigned char* va = im + (k0 < STOK ? k0 : 0) * ROW_B + voff;
        const unsigned char* vb = im + (k1 < STOK ? k1 : 0) * ROW_B + voff;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)va);
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)vb);
        f.vf[kt][sidx] = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
  };
  // one head of the pair from its fragments; its O rows are staged over the head's Q bytes of `im`
  auto head = [&](unsigned char* im, const f32x16 (&sa)[2][2], int h2, const Frags& f) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int qi = qt * 32 + r;  // this lane's query (local index)
      f32x16 s[2];                 // the scaled bias rows start this query tile's S
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        s[kt] = sa[qt][kt];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.kf[kt][ks], f.qf[qt][ks], s[kt], 0, 0, 0);
      }
      float m4[4] = {-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
          const float v = s[kt][rg] * scale;
          s[kt][rg] = v;
          m4[rg & 3] = fmaxf(m4[rg & 3], v);
        }
      float mloc = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
      mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
      const float ml = mloc * L2E;
      float p4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][rg], L2E, -ml));
          s[kt][rg] = p;
          p4[rg & 3] += p;
        }
      float psum = (p4[0] + p4[1]) + (p4[2] + p4[3]);
      psum += __shfl_xor(psum, 32, 64);
      // O^T = V^T . P^T
      f32x16 o = {0};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int sidx = 0; sidx < 2; ++sidx) {
          const bf16x8 pf = __builtin_bit_cast(
              bf16x8, make_uint4(mmr::pack2bf(s[kt][8 * sidx], s[kt][8 * sidx + 1]), mmr::pack2bf(s[kt][8 * sidx + 2], s[kt][8 * sidx + 3]),
                                 mmr::pack2bf(s[kt][8 * sidx + 4], s[kt][8 * sidx + 5]), mmr::pack2bf(s[kt][8 * sidx + 6], s[kt][8 * sidx + 7])));
          o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.vf[kt][sidx], pf, o, 0, 0, 0);
        }
      if (qi < STOK) {
        const float inv = 1.0f / psum;
        unsigned char* orow = im + qi * ROW_B + h2 * 64 + 8 * hf;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
          lds_write_b64(orow + 16 * g4, mmr::pack2bf(o[4 * g4] * inv, o[4 * g4 + 1] * inv),
                        mmr::pack2bf(o[4 * g4 + 2] * inv, o[4 * g4 + 3] * inv));
      }
    }
  };
  // the pair's 49 x 128 B of output staged in `im`: 16-B chunks, 8 lanes per 128-B segment, through
  // the reverse roll
  auto store_out = [&](const Unit& un, const unsigned char* im) {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < NOST; ++j) {
      const int c = j * 64 + lane, cc = c < OCH ? c : OCH - 1;
      const int t = cc >> 3, u8 = cc & 7;
      const uint4 v = *(const uint4*)(im + t * ROW_B + u8 * 16);
      const uint32_t row = img_row(un.hs, un.ws_, t / SWS, t % SWS);
      if (c < OCH) *(uint4*)(out + ((un.tok0 + row) * (uint32_t)C + (uint32_t)(un.hp * 64 + u8 * 8))) = v;
    }
  };

  Unit ud = unit_of(i0), pd = ud;
  bool have_prev = false;
  int buf = 0, cur = -1;
  f32x16 bsc[2][2][2];  // [head][qt][kt]: the current (window, head pair)'s bias rows * sqrt(dh)
  gather(ud, img0);
  for (int i = i0; i < i1; ++i) {
    unsigned char* im = img0 + buf * IMG_B;
    unsigned char* other = img0 + (buf ^ 1) * IMG_B;
    if (ud.combo != cur) {
      cur = ud.combo;
      load_bias(bsc[0], ud, 0);
      load_bias(bsc[1], ud, 1);
    }
    __builtin_amdgcn_s_waitcnt(vmcnt_n(0));  // this unit's image (issued one unit ago)
    asm volatile("" ::: "memory");
    if (have_prev) store_out(pd, other);
    Frags fr[2];
    read_frags(im, 0, fr[0]);
    read_frags(im, 1, fr[1]);
    __builtin_amdgcn_s_waitcnt(LGKM0);  // lgkmcnt(0): also `other` read out before the DMA writes it
    asm volatile("" ::: "memory");
    const bool more = i + 1 < i1;
    const Unit nd = more ? unit_of(i + 1) : ud;
    if (more) gather(nd, other);
    __builtin_amdgcn_sched_barrier(0);
    head(im, bsc[0], 0, fr[0]);
    head(im, bsc[1], 1, fr[1]);
    pd = ud;
    ud = nd;
    have_prev = true;
    buf ^= 1;
  }
  store_out(pd, img0 + (buf ^ 1) * IMG_B);
  __builtin_amdgcn_s_waitcnt(vmcnt_n(0));
}

}  // namespace

namespace mmr {

bool swa_stream_takes(int64_t b, int hw, int c, int heads, int ws) {
  const int64_t units = b * (hw / SWS) * (hw / SWS) * (heads / 2);
  return ws == SWS && hw % SWS == 0 && heads % 2 == 0 && c == heads * 32 && c <= 2048 && units > 0 &&
         units < ((int64_t)1 << 31) && b * hw * hw * 3 * c < ((int64_t)1 << 32);
}

bool swa_stream_auto(int64_t b, int hw, int heads) {
  // measured faster than the gather kernel from 3 units per wave up (profiles/r07_swa_stream_ab.txt: stage 4
  // at B = 256 is that point, a tie); smaller launches were not measured and stay where they were
  const int64_t units = b * (hw / SWS) * (hw / SWS) * (heads / 2);
  return units >= 3 * (int64_t)cu_count() * SWA_STREAM_WAVES;
}

mmr_status swa_stream_launch(const uint16_t* qkv, const float* bias, uint16_t* out, int32_t b, int32_t hw, int32_t c,
                             int32_t heads, int32_t shift, void* stream) {
  const int64_t units = (int64_t)b * (hw / SWS) * (hw / SWS) * (heads / 2);
  const int64_t grid = swa_stream_grid(units, cu_count());
  swin_wattn_stream<<<dim3((unsigned)grid), NW * 64, LDS_B, as_stream(stream)>>>(qkv, bias, out, (int)units, b, hw, c,
                                                                                 heads, shift);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

}  // namespace mmr
