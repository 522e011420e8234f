// The attention family of the reference's ExplanationEngine.explain (src/Model/explain.py:825-947) on device: from
// the last fusion layer's head-averaged maps txt2img (B, Lt, Np), img2txt (B, Np, Lt) and comb (B, Lc, Lc) the
// per-patch / per-token vectors, their weighted and min-max normalised combinations and the bilinear heat maps —
// forward-only arithmetic, for every sample of the batch (the reference maps sample 0 only).
//
// ex_vectors, one workgroup per sample:
//   p_txt  = column mean of txt2img                                   (txt2img_to_patch_vector, :715-719)
//   t_img  = column mean of img2txt                                   (img2txt_to_token_vector, :733-737)
//   p_comb = _comb_helper(comb, Np, 0.06, swap=False)   (:739-798)    Lc == Np: column mean; Lc > Np: the window of
//            Np consecutive columns with the largest mass (f64 column sums, ties: the lowest offset), all zeros when
//            max / (total + 1e-12) < 0.06, else the chosen columns' means; Lc < Np: absent (the host's decision)
//   t_comb = the first two steps of compute_comb_token_vector (:546-566): Lc == T: column mean; Lc > T: the same
//            search over row sums (T rows, ratio 0.0), the chosen rows' means; Lc < T: _attn_to_token_tensor
//            (:645-695) — row means, min-max normalised to [0, 1], the uniform 1 / Lc when |max - min| < 1e-8
//   final_patch = minmax(0.6 p_txt + 0.4 p_comb) (or the one that exists), final_token the same from t_img and
//            t_comb trimmed to the shorter                            (:886-935)
// Every mean is an f64 sum in a fixed order, divided and rounded to f32 once; what follows is f32 with contraction
// off.  No float atomics: two runs give identical bytes.
// ex_heat, workgroups (pixel chunk, map, sample): compute_attention_map (:87-102) — v = (x - min) / ((max - min) +
// 1e-8f) viewed G x G (G^2 = Np), bilinear to (H, W) as F.interpolate(align_corners=False) does in f32:
// src = (dst + 0.5) (G / out) - 0.5 clamped below at 0, neighbour index clamped at G - 1.  (The reference's second
// upscale_heatmap to the same size is the identity and is not run.)  4 consecutive pixels per thread, one 16-B store
// — where H W is a multiple of 4, so that every sample's map starts 16-B aligned (224 x 224, 28 x 28, ...); any other
// H W takes scalar stores for the whole map.
#include "bilinear.h"
#include "common.h"

#pragma clang fp contract(off)

namespace {

using mmr::aligned16;

constexpr int EX_MAXNP = 1024;  // patches (LDS vectors of the heat-map kernel)
constexpr int EX_MAXL = 4096;   // Lt, Lc (LDS token vectors)

struct ExSm {
  double part[256];
  double redd[4];
  float redf[4];
  int redi[4];
};

// 256 threads -> every thread the sum, in the wave_sum tree and then waves 0..3 in order
__device__ __forceinline__ double ex_block_sum(double v, ExSm& sm) {
  v = mmr::wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm.redd[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((sm.redd[0] + sm.redd[1]) + sm.redd[2]) + sm.redd[3];
  __syncthreads();
  return r;
}
template <bool MAX>
__device__ __forceinline__ float ex_block_ext(float v, ExSm& sm) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float o = __shfl_xor(v, m, 64);
    v = MAX ? fmaxf(v, o) : fminf(v, o);
  }
  if ((threadIdx.x & 63) == 0) sm.redf[threadIdx.x >> 6] = v;
  __syncthreads();
  const float a = MAX ? fmaxf(sm.redf[0], sm.redf[1]) : fminf(sm.redf[0], sm.redf[1]);
  const float b = MAX ? fmaxf(sm.redf[2], sm.redf[3]) : fminf(sm.redf[2], sm.redf[3]);
  __syncthreads();
  return MAX ? fmaxf(a, b) : fminf(a, b);
}
__device__ __forceinline__ int ex_block_count(int v, ExSm& sm) {
  v = mmr::wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm.redi[threadIdx.x >> 6] = v;
  __syncthreads();
  const int r = sm.redi[0] + sm.redi[1] + sm.redi[2] + sm.redi[3];
  __syncthreads();
  return r;
}
// min and max of v[0 .. n) (LDS)
__device__ __forceinline__ void ex_minmax(const float* v, int n, ExSm& sm, float& mn, float& mx) {
  float a = INFINITY, b = -INFINITY;
  for (int i = threadIdx.x; i < n; i += 256) {
    a = fminf(a, v[i]);
    b = fmaxf(b, v[i]);
  }
  mn = ex_block_ext<false>(a, sm);
  mx = ex_block_ext<true>(b, sm);
}

// the columns [0, cols) of a (rows x cols) matrix at row stride rs, summed over the rows in f64: dsum[c] = the sum
// (when given), mean[c] = (float)(sum / rows) (when given).  cols <= 128: 256 / cols row groups (group g: rows g,
// g + groups, ... in order), the groups added in order; wider: thread per column, rows in order
__device__ __forceinline__ void ex_col_sums(const float* __restrict__ m, int64_t rs, int rows, int cols,
                                            double* __restrict__ dsum, float* __restrict__ mean, ExSm& sm) {
  const int tid = threadIdx.x;
  if (cols <= 128) {
    const int groups = 256 / cols, g = tid / cols, c = tid - g * cols;
    double s = 0.0;
    if (g < groups)
      for (int r = g; r < rows; r += groups) s += (double)m[(int64_t)r * rs + c];
    sm.part[tid] = s;
    __syncthreads();
    if (tid < cols) {
      double t = 0.0;
      for (int k = 0; k < groups; ++k) t += sm.part[k * cols + tid];
      if (dsum) dsum[tid] = t;
      if (mean) mean[tid] = (float)(t / (double)rows);
    }
  } else {
    for (int c = tid; c < cols; c += 256) {
      double s = 0.0;
      for (int r = 0; r < rows; ++r) s += (double)m[(int64_t)r * rs + c];
      if (dsum) dsum[c] = s;
      if (mean) mean[c] = (float)(s / (double)rows);
    }
  }
  __syncthreads();
}
// dsum[r] = the f64 sum of row r's cols entries: wave per row, lane-strided then the wave_sum tree
__device__ __forceinline__ void ex_row_sums(const float* __restrict__ m, int64_t rs, int rows, int cols,
                                            double* __restrict__ dsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < rows; r += 4) {
    double s = 0.0;
    for (int c = lane; c < cols; c += 64) s += (double)m[(int64_t)r * rs + c];
    s = mmr::wave_sum(s);
    if (lane == 0) dsum[r] = s;
  }
  __syncthreads();
}
// over the len - n + 1 windows of n consecutive entries of s (each summed in order): the largest sum and its lowest
// offset; returns whether best / (total + 1e-12) < ratio (total = the sum of s).  off stays inside [0, len - n]
// whatever the values (NaN sums never win)
__device__ __forceinline__ bool ex_window(const double* __restrict__ s, int len, int n, double ratio, ExSm& sm,
                                          int& off) {
  constexpr int NONE = 0x7FFFFFFF;
  double bv = -INFINITY, tot = 0.0;
  int bo = NONE;
  for (int o = threadIdx.x; o + n <= len; o += 256) {
    double w = 0.0;
    for (int j = 0; j < n; ++j) w += s[o + j];
    if (w > bv) {
      bv = w;
      bo = o;
    }
  }
  for (int i = threadIdx.x; i < len; i += 256) tot += s[i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double v2 = __shfl_xor(bv, m, 64);
    const int o2 = __shfl_xor(bo, m, 64);
    if (v2 > bv || (v2 == bv && o2 < bo)) {
      bv = v2;
      bo = o2;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    sm.redd[threadIdx.x >> 6] = bv;
    sm.redi[threadIdx.x >> 6] = bo;
  }
  __syncthreads();
  bv = sm.redd[0];
  bo = sm.redi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (sm.redd[w] > bv || (sm.redd[w] == bv && sm.redi[w] < bo)) {
      bv = sm.redd[w];
      bo = sm.redi[w];
    }
  __syncthreads();
  const double total = ex_block_sum(tot, sm);
  off = bo == NONE ? 0 : bo;
  return bv / (total + 1e-12) < ratio;
}

// out = minmax(0.6 a + 0.4 b) over n entries, or minmax of the one given; a, b, tmp: LDS
__device__ __forceinline__ void ex_final(const float* a, const float* b, int n, float* tmp, float* __restrict__ out,
                                         ExSm& sm) {
  for (int i = threadIdx.x; i < n; i += 256) tmp[i] = a && b ? 0.6f * a[i] + 0.4f * b[i] : (a ? a[i] : b[i]);
  __syncthreads();
  float mn, mx;
  ex_minmax(tmp, n, sm, mn, mx);
  const float den = (mx - mn) + 1e-8f;
  for (int i = threadIdx.x; i < n; i += 256) out[i] = (tmp[i] - mn) / den;
}

struct ExArgs {
  const float *t2i, *i2t, *comb;
  int64_t t2i_bs, t2i_rs, i2t_bs, i2t_rs, comb_bs, comb_rs;
  int lt, np, lc, t;
  float *p_txt, *t_img, *p_comb, *t_comb, *final_patch, *final_token;
  int32_t* offsets;
  float* comb_absmax;
  unsigned long long* nonfinite;
  double* work;
};

__global__ __launch_bounds__(256) void ex_vectors(const ExArgs a) {
  __shared__ ExSm sm;
  __shared__ float pt[EX_MAXNP], pc[EX_MAXNP], ti[EX_MAXL], tc[EX_MAXL];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int np = a.np, lt = a.lt, lc = a.lc, t = a.t;
  const bool has_pc = a.comb && lc >= np;
  const int ltc = lc >= t ? t : lc;  // t_comb's length
  int bad = 0, off_p = -1, off_t = -1;
  if (a.t2i) {
    ex_col_sums(a.t2i + b * a.t2i_bs, a.t2i_rs, lt, np, nullptr, pt, sm);
    for (int i = tid; i < np; i += 256) {
      a.p_txt[(int64_t)b * np + i] = pt[i];
      bad += !isfinite(pt[i]);
    }
  }
  if (a.i2t) {
    ex_col_sums(a.i2t + b * a.i2t_bs, a.i2t_rs, np, lt, nullptr, ti, sm);
    for (int i = tid; i < lt; i += 256) {
      a.t_img[(int64_t)b * lt + i] = ti[i];
      bad += !isfinite(ti[i]);
    }
  }
  if (a.comb) {
    const float* cm = a.comb + b * a.comb_bs;
    double* ds = a.work + (int64_t)b * lc;  // this sample's f64 column, then row, sums
    if (lc == np) {
      ex_col_sums(cm, a.comb_rs, lc, np, nullptr, pc, sm);
      off_p = 0;
    } else if (lc > np) {
      ex_col_sums(cm, a.comb_rs, lc, lc, ds, nullptr, sm);
      const bool below = ex_window(ds, lc, np, 0.06, sm, off_p);
      for (int i = tid; i < np; i += 256) pc[i] = below ? 0.0f : (float)(ds[off_p + i] / (double)lc);
      __syncthreads();
    }
    if (lc == t) {
      ex_col_sums(cm, a.comb_rs, lc, t, nullptr, tc, sm);
      off_t = 0;
    } else {
      ex_row_sums(cm, a.comb_rs, lc, lc, ds);
      if (lc > t) {
        const bool below = ex_window(ds, lc, t, 0.0, sm, off_t);
        for (int i = tid; i < t; i += 256) tc[i] = below ? 0.0f : (float)(ds[off_t + i] / (double)lc);
        __syncthreads();
      } else {
        for (int i = tid; i < lc; i += 256) tc[i] = (float)(ds[i] / (double)lc);
        __syncthreads();
        float mn, mx;
        ex_minmax(tc, lc, sm, mn, mx);
        const float range = mx - mn;
        const bool uniform = fabsf(range) < 1e-8f;
        const float den = range + 1e-8f, u = 1.0f / (float)lc;
        for (int i = tid; i < lc; i += 256) {
          const float v = (tc[i] - mn) / den;
          tc[i] = uniform ? u : fminf(fmaxf(v, 0.0f), 1.0f);
        }
        __syncthreads();
      }
    }
    float am_p = 0.0f, am_t = 0.0f;
    if (has_pc)
      for (int i = tid; i < np; i += 256) {
        a.p_comb[(int64_t)b * np + i] = pc[i];
        bad += !isfinite(pc[i]);
        am_p = fmaxf(am_p, fabsf(pc[i]));
      }
    for (int i = tid; i < ltc; i += 256) {
      a.t_comb[(int64_t)b * ltc + i] = tc[i];
      bad += !isfinite(tc[i]);
      am_t = fmaxf(am_t, fabsf(tc[i]));
    }
    am_p = ex_block_ext<true>(am_p, sm);
    am_t = ex_block_ext<true>(am_t, sm);
    if (tid == 0) {
      a.comb_absmax[2 * b] = am_p;
      a.comb_absmax[2 * b + 1] = am_t;
    }
  }
  if (tid == 0) {
    a.offsets[2 * b] = off_p;
    a.offsets[2 * b + 1] = off_t;
  }
  if (a.t2i || has_pc) {
    // 0.6 p_txt + 0.4 p_comb in place (or the one that exists), normalised into final_patch
    const float* x = a.t2i ? pt : nullptr;
    const float* y = has_pc ? pc : nullptr;
    float* dst = a.t2i ? pt : pc;
    ex_final(x, y, np, dst, a.final_patch + (int64_t)b * np, sm);
  }
  if (a.i2t || a.comb) {
    const int n = a.i2t && a.comb ? (lt < ltc ? lt : ltc) : (a.i2t ? lt : ltc);
    const float* x = a.i2t ? ti : nullptr;
    const float* y = a.comb ? tc : nullptr;
    float* dst = a.i2t ? ti : tc;
    ex_final(x, y, n, dst, a.final_token + (int64_t)b * n, sm);
  }
  const int nbad = ex_block_count(bad, sm);
  if (tid == 0 && nbad) atomicAdd(a.nonfinite, (unsigned long long)nbad);
}

struct ExHeat {
  const float* src[3];  // (B, Np) vectors; NULL: no such map
  float* dst[3];        // (B, H, W)
  int np, g, h, w;
  float sh, sw;  // (float)G / H, (float)G / W
};

__global__ __launch_bounds__(256) void ex_heat(const ExHeat a) {
  __shared__ ExSm sm;
  __shared__ float v[EX_MAXNP];
  const int k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const float* src = a.src[k];
  if (!src) return;  // uniform over the workgroup
  for (int i = tid; i < a.np; i += 256) v[i] = src[(int64_t)b * a.np + i];
  __syncthreads();
  float mn, mx;
  ex_minmax(v, a.np, sm, mn, mx);
  const float den = (mx - mn) + 1e-8f;
  for (int i = tid; i < a.np; i += 256) v[i] = (v[i] - mn) / den;
  __syncthreads();
  const int hw = a.h * a.w, g = a.g;
  float* dst = a.dst[k] + (int64_t)b * hw;
  const bool vec = (hw & 3) == 0;  // then every sample's map starts 16-B aligned (dst is)
  for (int p0 = (blockIdx.x * 256 + tid) * 4; p0 < hw; p0 += gridDim.x * 1024) {
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + j < hw ? p0 + j : hw - 1;
      const int y = p / a.w, x = p - y * a.w;
      o[j] = mmr::bilinear_at(v, g, y, x, a.sh, a.sw);
    }
    if (vec) {
      *reinterpret_cast<float4*>(dst + p0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (p0 + j < hw) dst[p0 + j] = o[j];
    }
  }
}

inline bool ex_shape_ok(int32_t b, int32_t lt, int32_t np, int32_t lc) {
  return b >= 0 && lt >= 1 && lt <= EX_MAXL && np >= 1 && np <= EX_MAXNP && lc >= 0 && lc <= EX_MAXL;
}

}  // namespace

extern "C" {

int64_t mmr_explain_attention_work_bytes(int32_t b, int32_t lt, int32_t np, int32_t lc) {
  if (!ex_shape_ok(b, lt, np, lc)) return 0;
  const int64_t n = (int64_t)b * lc * 8;
  return n > 256 ? mmr::round_up(n, 256) : 256;
}

mmr_status mmr_explain_attention(const float* txt2img, int64_t t2i_bs, int64_t t2i_rs, const float* img2txt,
                                 int64_t i2t_bs, int64_t i2t_rs, const float* comb, int64_t comb_bs, int64_t comb_rs,
                                 int32_t b, int32_t lt, int32_t np, int32_t lc_rows, int32_t lc_cols, int32_t t,
                                 int32_t h, int32_t w, float* p_txt, float* t_img, float* p_comb, float* t_comb,
                                 float* final_patch, float* final_token, float* map_txt2img, float* map_comb,
                                 float* map_final, int32_t* offsets, float* comb_absmax, int64_t* nonfinite,
                                 void* work, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(b >= 0, "mmr_explain_attention: b = %d < 0", b);
  MMR_REQUIRE(np >= 1 && np <= EX_MAXNP, "mmr_explain_attention: Np = %d outside 1..%d", np, EX_MAXNP);
  MMR_REQUIRE(lt >= 1 && lt <= EX_MAXL, "mmr_explain_attention: Lt = %d outside 1..%d", lt, EX_MAXL);
  MMR_REQUIRE(t >= 1, "mmr_explain_attention: T = %d < 1", t);
  MMR_REQUIRE(txt2img || img2txt || comb, "mmr_explain_attention: all three maps are NULL");
  if (comb) {
    MMR_REQUIRE(lc_rows == lc_cols, "mmr_explain_attention: comb is %d x %d, not square", lc_rows, lc_cols);
    MMR_REQUIRE(lc_rows >= 1 && lc_rows <= EX_MAXL, "mmr_explain_attention: Lc = %d outside 1..%d", lc_rows, EX_MAXL);
    MMR_REQUIRE(comb_rs >= lc_cols, "mmr_explain_attention: comb row stride %lld < Lc = %d", (long long)comb_rs,
                lc_cols);
  }
  const int lc = comb ? lc_rows : 0;
  MMR_REQUIRE(!txt2img || t2i_rs >= np, "mmr_explain_attention: txt2img row stride %lld < Np = %d", (long long)t2i_rs,
              np);
  MMR_REQUIRE(!img2txt || i2t_rs >= lt, "mmr_explain_attention: img2txt row stride %lld < Lt = %d", (long long)i2t_rs,
              lt);
  const bool has_pc = comb && lc >= np;
  MMR_REQUIRE((!txt2img || p_txt) && (!img2txt || t_img) && (!has_pc || p_comb) && (!comb || t_comb),
              "mmr_explain_attention: NULL vector output for a map that is given");
  MMR_REQUIRE((!(txt2img || has_pc) || final_patch) && (!(img2txt || comb) || final_token),
              "mmr_explain_attention: NULL final_patch / final_token");
  MMR_REQUIRE(offsets && nonfinite && (!comb || comb_absmax), "mmr_explain_attention: NULL offsets / comb_absmax / "
              "nonfinite");
  MMR_REQUIRE(!comb || (work && aligned16(work)), "mmr_explain_attention: work is NULL or not 16-B aligned");
  MMR_REQUIRE(!map_txt2img || txt2img, "mmr_explain_attention: map_txt2img without txt2img");
  MMR_REQUIRE(!map_comb || has_pc, "mmr_explain_attention: map_comb without a comb patch vector (Lc >= Np)");
  MMR_REQUIRE(!map_final || txt2img || has_pc, "mmr_explain_attention: map_final without a patch vector");
  const bool heat = map_txt2img || map_comb || map_final;
  int g = 0;
  if (heat) {
    while (g * g < np) ++g;
    MMR_REQUIRE(g * g == np, "mmr_explain_attention: Np = %d is not a perfect square (heat maps are G x G)", np);
    MMR_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= 65536, "mmr_explain_attention: H x W = %d x %d outside 1..65536 "
                "pixels", h, w);
    MMR_REQUIRE((!map_txt2img || aligned16(map_txt2img)) && (!map_comb || aligned16(map_comb)) &&
                (!map_final || aligned16(map_final)), "mmr_explain_attention: a heat map is not 16-B aligned");
  }
  hipStream_t st = mmr::as_stream(stream);
  MMR_CHECK_HIP(hipMemsetAsync(nonfinite, 0, sizeof(int64_t), st));
  if (b == 0) return MMR_OK;
  MMR_REQUIRE(b <= mmr::MAX_GRID_Y, "mmr_explain_attention: b = %d > %d", b, mmr::MAX_GRID_Y);
  ExArgs a;
  a.t2i = txt2img, a.i2t = img2txt, a.comb = comb;
  a.t2i_bs = t2i_bs, a.t2i_rs = t2i_rs, a.i2t_bs = i2t_bs, a.i2t_rs = i2t_rs, a.comb_bs = comb_bs, a.comb_rs = comb_rs;
  a.lt = lt, a.np = np, a.lc = lc, a.t = t;
  a.p_txt = p_txt, a.t_img = t_img, a.p_comb = p_comb, a.t_comb = t_comb;
  a.final_patch = final_patch, a.final_token = final_token;
  a.offsets = offsets, a.comb_absmax = comb_absmax, a.nonfinite = (unsigned long long*)nonfinite;
  a.work = (double*)work;
  ex_vectors<<<dim3((unsigned)b), 256, 0, st>>>(a);
  if (heat) {
    ExHeat e;
    e.src[0] = map_txt2img ? p_txt : nullptr, e.dst[0] = map_txt2img;
    e.src[1] = map_comb ? p_comb : nullptr, e.dst[1] = map_comb;
    e.src[2] = map_final ? final_patch : nullptr, e.dst[2] = map_final;
    e.np = np, e.g = g, e.h = h, e.w = w;
    e.sh = (float)g / (float)h, e.sw = (float)g / (float)w;
    const int64_t chunks = mmr::ceil_div((int64_t)h * w, 1024);
    ex_heat<<<dim3((unsigned)(chunks < 16 ? chunks : 16), 3, (unsigned)b), 256, 0, st>>>(e);
  }
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

}  // extern "C"
