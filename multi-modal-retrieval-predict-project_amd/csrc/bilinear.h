// Bilinear resampling of a G x G grid to (H, W) as F.interpolate(mode="bilinear", align_corners=False) does in f32:
// src = (dst + 0.5) (G / out) - 0.5 clamped below at 0, neighbour index clamped at G - 1.  One definition for the
// attention heat maps (explain.hip) and the gradient maps (explain_grad.hip): the same expression, so the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace mmr {

__device__ __forceinline__ void bilinear_src(int d, float scale, int g, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
  float s = ((float)d + 0.5f) * scale - 0.5f;
  s = s < 0.0f ? 0.0f : s;
  i0 = (int)s;
  i0 = i0 < g - 1 ? i0 : g - 1;
  i1 = i0 < g - 1 ? i0 + 1 : i0;
  l1 = s - (float)i0;
}

// the (h, w) map's pixel (y, x) from the g x g grid v; sh = (float)g / h, sw = (float)g / w
__device__ __forceinline__ float bilinear_at(const float* v, int g, int y, int x, float sh, float sw) {
#pragma clang fp contract(off)
  int y0, y1, x0, x1;
  float ly, lx;
  bilinear_src(y, sh, g, y0, y1, ly);
  bilinear_src(x, sw, g, x0, x1, lx);
  const float hy = 1.0f - ly, hx = 1.0f - lx;
  return hy * (hx * v[y0 * g + x0] + lx * v[y0 * g + x1]) + ly * (hx * v[y1 * g + x0] + lx * v[y1 * g + x1]);
}

}  // namespace mmr
