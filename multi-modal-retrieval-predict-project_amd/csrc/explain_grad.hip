// The gradient family of the reference's ExplanationEngine (src/Model/explain.py:170-427, Grad-CAM and Integrated
// Gradients over the image patch features) needs the backward of ONE CrossModalFusion layer plus the classifier: a
// fixed graph of linears, LayerNorms, softmax attentions and a GELU.  The linear data gradients are the existing
// f32 linears on transposed weights; this file holds the rest, f32 throughout, every sum in a fixed order, no
// floating-point atomics (two runs, and a sequence alone or inside a larger launch, give identical bytes):
//
// ab_attention<DHT, FWD>  one workgroup (4 waves) per (sequence, head).  K and V (lk x dh, zero-padded to multiples
//   of 16) stay in LDS; the query side goes through in tiles of 16 rows: Q and dO tiles, S = scale Q K^T and
//   dP = dO V^T (16 x lk) in LDS, the softmax P = softmax(S) recomputed (the forward saves no probabilities) and
//   dS = P o (dP - rowsum(dP o P)) in place, then dV += P^T dO and dK += dS^T Q into MFMA accumulators that live
//   across the tiles (wave w owns key blocks w and w + 4), dQ = scale dS K per tile.  Every contraction is the
//   f32-input MFMA v_mfma_f32_16x16x4_f32.  FWD: the same walk writes O = P V instead (the f32 forward of the
//   gradient pass; mmr_x3_attention's bf16x3 scores are ~2^-17 per product, above the maps' error bound).
//   LDS at lk = 128, dh = 96: K, V 2 x 128 x 100 x 4 = 100 KB, Q / dO tiles 12.5 KB, S / dP tiles 16.5 KB: 129 KB of
//   the 160 KB (rows padded by 4 floats: the MFMA operand reads, 16 rows x 4 columns per instruction, then hit 64
//   distinct banks).
// lb_rows    LayerNorm backward, a wave per row: dz = rstd (g^ - mean(g^) - z^ mean(g^ o z^)), g^ = gamma o dy
// gb_rows    dx = dy gelu'(h), gelu'(h) = Phi(h) + h phi(h) with the exact erf form (ocml erff / expf); optionally
//            y = gelu(h) by the same erff
// am_raw / am_map   the per-patch attribution vectors and the finished (H, W) maps (below)
#include "bilinear.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

using mmr::aligned16;
using mmr::f32x4;

constexpr int AB_MAXL = 128;   // lq, lk
constexpr int AB_MAXDH = 96;   // head width
constexpr int AB_QT = 16;      // query rows per tile
constexpr int AM_MAXNP = 1024;
constexpr int AM_MAXSTEPS = 1024;

struct AbArgs {
  const float *q, *k, *v, *go;
  float *dq, *dk, *dv;  // FWD: dq = out
  int64_t ldq, ldk, ldv, ldo, lddq, lddk, lddv;
  int lq, lk, heads, dh;
  float scale;
};

inline int ab_lkp(int lk) { return (lk + 15) / 16 * 16; }
inline size_t ab_lds_bytes(int lk, int dht) {
  const int ks = dht * 16 + 4, ss = ab_lkp(lk) + 4;
  return (size_t)((2 * ab_lkp(lk) + 2 * AB_QT) * ks + 2 * AB_QT * ss) * sizeof(float);
}

// rows [r0, r0 + nrows) x columns [0, dhp) of a head's strided rows -> LDS rows of stride ks; rows >= rmax and columns
// >= dh read as zero
__device__ __forceinline__ void ab_stage(float* dst, const float* src, int64_t ld, int r0, int nrows, int rmax, int dh,
                                         int dhp, int ks) {
  const int q4 = dhp / 4;
  for (int i = threadIdx.x; i < nrows * q4; i += 256) {
    const int r = i / q4, c = (i - r * q4) * 4;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < rmax && c < dh) val = *reinterpret_cast<const float4*>(src + (int64_t)(r0 + r) * ld + c);
    *reinterpret_cast<float4*>(dst + r * ks + c) = val;
  }
}

template <int DHT, bool FWD>
__global__ __launch_bounds__(256) void ab_attention(const AbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int DHP = DHT * 16, KS = DHP + 4;
  const int lq = a.lq, lk = a.lk, dh = a.dh;
  const int lkp = (lk + 15) / 16 * 16, ss = lkp + 4;
  float* Ks = reinterpret_cast<float*>(smem);
  float* Vs = Ks + lkp * KS;
  float* Qs = Vs + lkp * KS;
  float* Gs = Qs + AB_QT * KS;
  float* Ss = Gs + AB_QT * KS;
  float* Ds = Ss + AB_QT * ss;
  const int seq = blockIdx.x / a.heads, head = blockIdx.x - seq * a.heads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, l4 = lane >> 4;
  const int64_t hoff = (int64_t)head * dh;
  const bool want_dk = !FWD && a.dk, want_dv = !FWD && a.dv, want_dq = FWD || a.dq;
  const bool want_ds = !FWD && (a.dk || a.dq);

  ab_stage(Ks, a.k + (int64_t)seq * lk * a.ldk + hoff, a.ldk, 0, lkp, lk, dh, DHP, KS);
  ab_stage(Vs, a.v + (int64_t)seq * lk * a.ldv + hoff, a.ldv, 0, lkp, lk, dh, DHP, KS);

  f32x4 acc_k[2][DHT], acc_v[2][DHT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < DHT; ++j) acc_k[i][j] = acc_v[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int q0 = 0; q0 < lq; q0 += AB_QT) {
    ab_stage(Qs, a.q + (int64_t)seq * lq * a.ldq + hoff, a.ldq, q0, AB_QT, lq, dh, DHP, KS);
    if (!FWD) ab_stage(Gs, a.go + (int64_t)seq * lq * a.ldo + hoff, a.ldo, q0, AB_QT, lq, dh, DHP, KS);
    __syncthreads();
    // S = scale Q K^T, dP = dO V^T: wave w the key blocks w, w + 4
#pragma unroll
    for (int kbi = 0; kbi < 2; ++kbi) {
      const int kb = wave + 4 * kbi;
      if (kb * 16 < lkp) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, p = {0.f, 0.f, 0.f, 0.f};
        const float* qa = Qs + l16 * KS + l4;
        const float* ga = Gs + l16 * KS + l4;
        const float* kr = Ks + (kb * 16 + l16) * KS + l4;
        const float* vr = Vs + (kb * 16 + l16) * KS + l4;
#pragma unroll
        for (int k0 = 0; k0 < DHP; k0 += 4) {
          s = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[k0], kr[k0], s, 0, 0, 0);
          if (!FWD) p = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[k0], vr[k0], p, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          Ss[(4 * l4 + i) * ss + kb * 16 + l16] = s[i] * a.scale;
          if (!FWD) Ds[(4 * l4 + i) * ss + kb * 16 + l16] = p[i];
        }
      }
    }
    __syncthreads();
    // softmax over the lk columns and dS, 16 threads (one DPP row) per query row
    {
      const int row = tid >> 4, j = tid & 15;
      float* sr = Ss + row * ss;
      float* dr = Ds + row * ss;
      float m = -INFINITY;
      for (int c = j; c < lkp; c += 16) m = fmaxf(m, c < lk ? sr[c] : -INFINITY);
      m = mmr::row16_max(m);
      float sum = 0.f;
      for (int c = j; c < lkp; c += 16) {
        const float e = c < lk ? expf(sr[c] - m) : 0.f;
        sr[c] = e;
        sum += e;
      }
      sum = mmr::row16_sum(sum);
      float dot = 0.f;
      for (int c = j; c < lkp; c += 16) {
        const float p = sr[c] / sum;
        sr[c] = p;
        if (!FWD) dot += p * dr[c];
      }
      if (want_ds) {
        dot = mmr::row16_sum(dot);
        for (int c = j; c < lkp; c += 16) dr[c] = sr[c] * (dr[c] - dot);  // padded columns: P = 0
      }
    }
    __syncthreads();
    if (!FWD && (want_dk || want_dv)) {
      // dV += P^T dO, dK += dS^T Q: the contraction runs over the tile's 16 query rows
#pragma unroll
      for (int kbi = 0; kbi < 2; ++kbi) {
        const int kb = wave + 4 * kbi;
        if (kb * 16 < lkp) {
#pragma unroll
          for (int k0 = 0; k0 < AB_QT; k0 += 4) {
            const float pa = Ss[(k0 + l4) * ss + kb * 16 + l16];
            const float da = Ds[(k0 + l4) * ss + kb * 16 + l16];
#pragma unroll
            for (int nt = 0; nt < DHT; ++nt) {
              if (want_dv)
                acc_v[kbi][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, Gs[(k0 + l4) * KS + nt * 16 + l16],
                                                                      acc_v[kbi][nt], 0, 0, 0);
              if (want_dk)
                acc_k[kbi][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(da, Qs[(k0 + l4) * KS + nt * 16 + l16],
                                                                      acc_k[kbi][nt], 0, 0, 0);
            }
          }
        }
      }
    }
    if (want_dq) {
      // dQ = scale dS K (FWD: O = P V): wave w the column tiles w, w + 4
      const float* lhs = FWD ? Ss : Ds;
      const float* rhs = FWD ? Vs : Ks;
      const float mul = FWD ? 1.0f : a.scale;
#pragma unroll
      for (int nti = 0; nti < 2; ++nti) {
        const int nt = wave + 4 * nti;
        if (nt < DHT) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          for (int k0 = 0; k0 < lkp; k0 += 4)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(lhs[l16 * ss + k0 + l4], rhs[(k0 + l4) * KS + nt * 16 + l16], acc,
                                                       0, 0, 0);
          const int col = nt * 16 + l16;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = q0 + 4 * l4 + i;
            if (r < lq && col < dh) a.dq[((int64_t)seq * lq + r) * a.lddq + hoff + col] = acc[i] * mul;
          }
        }
      }
    }
    __syncthreads();
  }
  if (!FWD) {
#pragma unroll
    for (int kbi = 0; kbi < 2; ++kbi) {
      const int kb = wave + 4 * kbi;
      if (kb * 16 < lkp) {
#pragma unroll
        for (int nt = 0; nt < DHT; ++nt) {
          const int col = nt * 16 + l16;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = kb * 16 + 4 * l4 + i;
            if (r < lk && col < dh) {
              if (want_dk) a.dk[((int64_t)seq * lk + r) * a.lddk + hoff + col] = acc_k[kbi][nt][i] * a.scale;
              if (want_dv) a.dv[((int64_t)seq * lk + r) * a.lddv + hoff + col] = acc_v[kbi][nt][i];
            }
          }
        }
      }
    }
  }
}

template <bool FWD>
mmr_status ab_launch(const char* name, const AbArgs& a, int b, hipStream_t st) {
  const int dht = (a.dh + 15) / 16;
  const size_t lds = ab_lds_bytes(a.lk, dht);
  if (lds > 160 * 1024) {  // cannot happen inside the limits checked by the callers
    mmr::set_error("%s: %zu bytes of LDS", name, lds);
    return MMR_ERR_UNSUPPORTED;
  }
  const dim3 grid((unsigned)((int64_t)b * a.heads));
  mmr::pick<1, 2, 3, 4, 5, 6>(dht, [&](auto t) {
    ab_attention<decltype(t)::value, FWD><<<grid, 256, lds, st>>>(a);
  });
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

// shape / operand checks shared by the forward and the backward; nothing is clamped
#define AB_CHECK_SHAPE(name)                                                                                          \
  do {                                                                                                                \
    MMR_REQUIRE(b >= 0 && heads >= 1, "%s: b = %d, heads = %d", name, b, heads);                                      \
    MMR_REQUIRE(q && k && v, "%s: NULL q / k / v", name);                                                             \
    if (lq < 1 || lq > AB_MAXL || lk < 1 || lk > AB_MAXL) {                                                           \
      mmr::set_error("%s: lq = %d, lk = %d outside 1..%d", name, lq, lk, AB_MAXL);                                    \
      return MMR_ERR_UNSUPPORTED;                                                                                     \
    }                                                                                                                 \
    if (dh < 8 || dh % 8 != 0 || dh > AB_MAXDH) {                                                                     \
      mmr::set_error("%s: head_dim %d is not a multiple of 8 in 8..%d", name, dh, AB_MAXDH);                          \
      return MMR_ERR_UNSUPPORTED;                                                                                     \
    }                                                                                                                 \
    MMR_REQUIRE((int64_t)b* heads <= 0x7FFFFFFFLL, "%s: b * heads = %lld workgroups", name, (long long)b* heads);     \
  } while (0)

inline bool ab_rows_ok(const void* p, int64_t ld, int heads, int dh) {
  return aligned16(p) && ld % 4 == 0 && ld >= (int64_t)heads * dh;
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm backward, a wave per row
__global__ __launch_bounds__(256) void lb_rows(const float* __restrict__ z, int64_t ldz, const float* __restrict__ gamma,
                                               const float* __restrict__ dy, int64_t lddy, float* __restrict__ dz,
                                               int64_t lddz, int64_t rows, int c, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // uniform over the wave
  const float* zr = z + r * ldz;
  const float* gr = dy + r * lddy;
  const float fc = (float)c;
  float s = 0.f;
  for (int i = lane; i < c; i += 64) s += zr[i];
  const float mean = mmr::wave_sum(s) / fc;
  s = 0.f;
  for (int i = lane; i < c; i += 64) {
    const float d = zr[i] - mean;
    s += d * d;
  }
  const float rstd = 1.0f / sqrtf(mmr::wave_sum(s) / fc + eps);
  float s1 = 0.f, s2 = 0.f;
  for (int i = lane; i < c; i += 64) {
    const float g = gamma[i] * gr[i], zh = (zr[i] - mean) * rstd;
    s1 += g;
    s2 += g * zh;
  }
  const float m1 = mmr::wave_sum(s1) / fc, m2 = mmr::wave_sum(s2) / fc;
  for (int i = lane; i < c; i += 64) {
    const float g = gamma[i] * gr[i], zh = (zr[i] - mean) * rstd;
    dz[r * lddz + i] = rstd * ((g - m1) - zh * m2);
  }
}

// GELU (erf form) backward and, optionally, forward
__global__ __launch_bounds__(256) void gb_rows(const float* __restrict__ h, int64_t ldh, const float* __restrict__ dy,
                                               int64_t lddy, float* __restrict__ dx, int64_t lddx, float* __restrict__ y,
                                               int64_t ldy, int64_t rows, int c) {
  const int64_t n = rows * c;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / c;
    const int col = (int)(i - r * c);
    const float x = h[r * ldh + col];
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
    if (y) y[r * ldy + col] = x * cdf;
    if (dx) {
      const float pdf = 0.39894228040143268f * expf(-0.5f * x * x);
      dx[r * lddx + col] = dy[r * lddy + col] * (cdf + x * pdf);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Attribution maps.  grad (maps * steps, np, ci): map m's rows are m * steps + s; map m reads the patch set
// x[(m / x_div) % x_mod] of x (.., np, ci).
// am_raw, a wave per (map, patch): raw = sum_e t_e (Grad-CAM, before the relu) or sum_e |t_e| (IG), t_e = (sum_s w_s
//   grad_s[e]) x[e] — the steps in order (w NULL: 1), then lanes e = lane, lane + 64, ... in order and the wave_sum
//   tree; these two sums of f32 products run in f64 and are rounded to f32 once (as explain.hip's means are): a
//   vector dominated by one patch is then the rounded sum of its f32 gradients, not that sum plus ~log2(steps ci)
//   roundings of its own.
// am_map, a workgroup per map: mode 0 (compute_gradcam_map_for_target, explain.py:274-300) relu, view G x G, bilinear
//   to (H, W), THEN (m - min) / ((max - min) + 1e-8f) over the pixels; mode 1 (compute_ig_map_for_target, :403-427)
//   (a - min) / ((max - min) + 1e-8f) over the patches, clamp to [0, 1], THEN bilinear.  Both end in nan_to_num(nan = 0,
//   posinf = 1, neginf = 0) where the reference has it (mode 0: the pixels; mode 1: the patch vector).
__global__ __launch_bounds__(256) void am_raw(const float* __restrict__ grad, const float* __restrict__ x,
                                              const float* __restrict__ w, float* __restrict__ raw, int64_t maps,
                                              int steps, int x_div, int x_mod, int np, int ci, int mode) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= maps * np) return;  // uniform over the wave
  const int64_t m = u / np;
  const int j = (int)(u - m * np);
  const float* g0 = grad + ((m * steps) * np + j) * (int64_t)ci;
  const float* xr = x + (((m / x_div) % x_mod) * np + j) * (int64_t)ci;
  const int64_t gs = (int64_t)np * ci;
  double part = 0.0;
  for (int e = lane; e < ci; e += 64) {
    double acc = 0.0;
    for (int s = 0; s < steps; ++s) acc += (double)(w ? w[s] : 1.0f) * (double)g0[s * gs + e];
    const double t = acc * (double)xr[e];
    part += mode ? fabs(t) : t;
  }
  part = mmr::wave_sum(part);
  if (lane == 0) raw[u] = (float)part;
}

struct AmSm {
  float lo[4], hi[4];
};
__device__ __forceinline__ void am_block_minmax(float& mn, float& mx, AmSm& sm) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, m, 64));
    mx = fmaxf(mx, __shfl_xor(mx, m, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    sm.lo[threadIdx.x >> 6] = mn;
    sm.hi[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(sm.lo[0], sm.lo[1]), fminf(sm.lo[2], sm.lo[3]));
  mx = fmaxf(fmaxf(sm.hi[0], sm.hi[1]), fmaxf(sm.hi[2], sm.hi[3]));
  __syncthreads();
}
__device__ __forceinline__ float am_nan_to_num(float v) {
  if (isnan(v)) return 0.0f;
  if (isinf(v)) return v > 0.0f ? 1.0f : 0.0f;
  return v;
}

__global__ __launch_bounds__(256) void am_map(const float* __restrict__ raw, float* __restrict__ out, int np, int g,
                                              int h, int w, float sh, float sw, int mode) {
  __shared__ AmSm sm;
  __shared__ float v[AM_MAXNP];
  const int tid = threadIdx.x, hw = h * w;
  const float* src = raw + (int64_t)blockIdx.x * np;
  float* dst = out + (int64_t)blockIdx.x * hw;
  for (int i = tid; i < np; i += 256) v[i] = mode ? src[i] : fmaxf(src[i], 0.0f);
  __syncthreads();
  float mn = INFINITY, mx = -INFINITY;
  if (mode) {
    for (int i = tid; i < np; i += 256) {
      mn = fminf(mn, v[i]);
      mx = fmaxf(mx, v[i]);
    }
    am_block_minmax(mn, mx, sm);
    const float den = (mx - mn) + 1e-8f;
    for (int i = tid; i < np; i += 256) v[i] = am_nan_to_num(fminf(fmaxf((v[i] - mn) / den, 0.0f), 1.0f));
    __syncthreads();
    for (int p = tid; p < hw; p += 256) {
      const int y = p / w;
      dst[p] = mmr::bilinear_at(v, g, y, p - y * w, sh, sw);
    }
  } else {
    for (int p = tid; p < hw; p += 256) {
      const int y = p / w;
      const float o = mmr::bilinear_at(v, g, y, p - y * w, sh, sw);
      mn = fminf(mn, o);
      mx = fmaxf(mx, o);
    }
    am_block_minmax(mn, mx, sm);
    const float den = (mx - mn) + 1e-8f;
    for (int p = tid; p < hw; p += 256) {  // the same expression again: the same bits as in the first pass
      const int y = p / w;
      const float o = mmr::bilinear_at(v, g, y, p - y * w, sh, sw);
      dst[p] = am_nan_to_num((o - mn) / den);
    }
  }
}

}  // namespace

extern "C" {

mmr_status mmr_attention_fwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                 float* out, int64_t ldo, int32_t b, int32_t lq, int32_t lk, int32_t heads, int32_t dh,
                                 float scale, void* stream) {
  mmr::clear_error();
  AB_CHECK_SHAPE("mmr_attention_fwd_f32");
  MMR_REQUIRE(out, "mmr_attention_fwd_f32: NULL out");
  MMR_REQUIRE(ab_rows_ok(q, ldq, heads, dh) && ab_rows_ok(k, ldk, heads, dh) && ab_rows_ok(v, ldv, heads, dh),
              "mmr_attention_fwd_f32: q / k / v need 16-B alignment and a row stride that is a multiple of 4 and >= "
              "heads * dh = %d", heads * dh);
  MMR_REQUIRE(ldo >= (int64_t)heads * dh, "mmr_attention_fwd_f32: out row stride %lld < heads * dh = %d", (long long)ldo,
              heads * dh);
  if (b == 0) return MMR_OK;
  AbArgs a{};
  a.q = q, a.k = k, a.v = v, a.go = nullptr, a.dq = out, a.dk = a.dv = nullptr;
  a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.lddq = ldo;
  a.lq = lq, a.lk = lk, a.heads = heads, a.dh = dh, a.scale = scale;
  return ab_launch<true>("mmr_attention_fwd_f32", a, b, mmr::as_stream(stream));
}

mmr_status mmr_attention_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                 const float* d_out, int64_t ldo, float* dq, int64_t lddq, float* dk, int64_t lddk,
                                 float* dv, int64_t lddv, int32_t b, int32_t lq, int32_t lk, int32_t heads, int32_t dh,
                                 float scale, void* stream) {
  mmr::clear_error();
  AB_CHECK_SHAPE("mmr_attention_bwd_f32");
  MMR_REQUIRE(d_out, "mmr_attention_bwd_f32: NULL d_out");
  MMR_REQUIRE(ab_rows_ok(q, ldq, heads, dh) && ab_rows_ok(k, ldk, heads, dh) && ab_rows_ok(v, ldv, heads, dh) &&
              ab_rows_ok(d_out, ldo, heads, dh),
              "mmr_attention_bwd_f32: q / k / v / d_out need 16-B alignment and a row stride that is a multiple of 4 "
              "and >= heads * dh = %d", heads * dh);
  const int64_t need = (int64_t)heads * dh;
  MMR_REQUIRE((!dq || lddq >= need) && (!dk || lddk >= need) && (!dv || lddv >= need),
              "mmr_attention_bwd_f32: an output row stride is < heads * dh = %lld", (long long)need);
  if (b == 0 || !(dq || dk || dv)) return MMR_OK;
  AbArgs a{};
  a.q = q, a.k = k, a.v = v, a.go = d_out, a.dq = dq, a.dk = dk, a.dv = dv;
  a.ldq = ldq, a.ldk = ldk, a.ldv = ldv, a.ldo = ldo, a.lddq = lddq, a.lddk = lddk, a.lddv = lddv;
  a.lq = lq, a.lk = lk, a.heads = heads, a.dh = dh, a.scale = scale;
  return ab_launch<false>("mmr_attention_bwd_f32", a, b, mmr::as_stream(stream));
}

mmr_status mmr_ln_bwd_rows(const float* z, int64_t ldz, const float* gamma, const float* dy, int64_t lddy, float* dz,
                           int64_t lddz, int64_t rows, int32_t c, float eps, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(z && gamma && dy && dz, "mmr_ln_bwd_rows: NULL z / gamma / dy / dz");
  MMR_REQUIRE(rows >= 0 && c >= 1 && c <= 1024, "mmr_ln_bwd_rows: rows = %lld, c = %d (c in 1..1024)", (long long)rows,
              c);
  MMR_REQUIRE(ldz >= c && lddy >= c && lddz >= c, "mmr_ln_bwd_rows: a row stride is < c = %d", c);
  if (rows == 0) return MMR_OK;
  const int64_t blocks = mmr::ceil_div(rows, 4);
  MMR_REQUIRE(blocks <= 0x7FFFFFFFLL, "mmr_ln_bwd_rows: %lld rows", (long long)rows);
  lb_rows<<<dim3((unsigned)blocks), 256, 0, mmr::as_stream(stream)>>>(z, ldz, gamma, dy, lddy, dz, lddz, rows, c, eps);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

mmr_status mmr_gelu_bwd_rows(const float* h, int64_t ldh, const float* dy, int64_t lddy, float* dx, int64_t lddx,
                             float* y, int64_t ldy, int64_t rows, int32_t c, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(h && (dx || y), "mmr_gelu_bwd_rows: NULL h, or neither dx nor y");
  MMR_REQUIRE(!dx || dy, "mmr_gelu_bwd_rows: dx without dy");
  MMR_REQUIRE(rows >= 0 && c >= 1, "mmr_gelu_bwd_rows: rows = %lld, c = %d", (long long)rows, c);
  MMR_REQUIRE(ldh >= c && (!dx || (lddy >= c && lddx >= c)) && (!y || ldy >= c),
              "mmr_gelu_bwd_rows: a row stride is < c = %d", c);
  if (rows == 0) return MMR_OK;
  const int64_t blocks = mmr::ceil_div(rows * c, 256);
  gb_rows<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), 256, 0, mmr::as_stream(stream)>>>(h, ldh, dy, lddy, dx, lddx,
                                                                                              y, ldy, rows, c);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

mmr_status mmr_attribution_maps(const float* grad, const float* x, const float* step_w, int64_t maps, int32_t steps,
                                int32_t x_div, int32_t x_mod, int32_t np, int32_t ci, int32_t mode, int32_t h, int32_t w,
                                float* raw,
                                float* out_maps, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(grad && x && raw, "mmr_attribution_maps: NULL grad / x / raw");
  MMR_REQUIRE(mode == 0 || mode == 1, "mmr_attribution_maps: mode %d (0 Grad-CAM, 1 Integrated Gradients)", mode);
  MMR_REQUIRE(maps >= 0 && steps >= 1 && steps <= AM_MAXSTEPS && x_div >= 1 && x_mod >= 1 && ci >= 1,
              "mmr_attribution_maps: maps = %lld, steps = %d (1..%d), x_div = %d, x_mod = %d, ci = %d", (long long)maps,
              steps, AM_MAXSTEPS, x_div, x_mod, ci);
  MMR_REQUIRE(np >= 1 && np <= AM_MAXNP, "mmr_attribution_maps: Np = %d outside 1..%d", np, AM_MAXNP);
  int g = 0;
  if (out_maps) {
    while (g * g < np) ++g;
    MMR_REQUIRE(g * g == np, "mmr_attribution_maps: Np = %d is not a perfect square (the maps are G x G)", np);
    MMR_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= 65536, "mmr_attribution_maps: H x W = %d x %d outside 1..65536 "
                "pixels", h, w);
  }
  if (maps == 0) return MMR_OK;
  const int64_t blocks = mmr::ceil_div(maps * np, 4);
  MMR_REQUIRE(blocks <= 0x7FFFFFFFLL && maps <= 0x7FFFFFFFLL, "mmr_attribution_maps: %lld maps", (long long)maps);
  hipStream_t st = mmr::as_stream(stream);
  am_raw<<<dim3((unsigned)blocks), 256, 0, st>>>(grad, x, step_w, raw, maps, steps, x_div, x_mod, np, ci, mode);
  if (out_maps)
    am_map<<<dim3((unsigned)maps), 256, 0, st>>>(raw, out_maps, np, g, h, w, (float)g / (float)h, (float)g / (float)w,
                                                 mode);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

}  // extern "C"
