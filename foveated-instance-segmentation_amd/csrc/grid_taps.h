// Bilinear taps of grid_sample (zeros padding, align_corners=False), shared by the sampler (frontend.hip: K5 / K6) and the
// un-warp (unwarp.hip: the sampled-space decisions).  Arithmetic follows the bit-exact recipe of SURVEY.md §8(a)-A12 (verified
// against ATen's CPU kernel by the goldens):
//   ix = fma(gx+1, W/2, -0.5); w = ix-floor(ix); weights nw=(1-n)(1-w) ...; acc = nw*v_nw;
//   acc = fma(v_ne,ne,acc); acc = fma(v_sw,sw,acc); acc = fma(v_se,se,acc).
// Explicit __f*_rn intrinsics keep hipcc from re-associating or contracting differently.
#pragma once
#include "common.h"

namespace {

struct Taps {
  int x0, y0;
  float nw, ne, sw, se;
  bool okx0, okx1, oky0, oky1;
  float w, n, e, s;   // fractional parts (east/south weights) and their complements
};
__device__ __forceinline__ Taps make_taps(float gx, float gy, int H, int W) {
  Taps t;
  const float ix = __fmaf_rn(__fadd_rn(gx, 1.f), (float)W * 0.5f, -0.5f);
  const float iy = __fmaf_rn(__fadd_rn(gy, 1.f), (float)H * 0.5f, -0.5f);
  const float fx = floorf(ix), fy = floorf(iy);
  t.w = __fsub_rn(ix, fx); t.e = __fsub_rn(1.f, t.w);
  t.n = __fsub_rn(iy, fy); t.s = __fsub_rn(1.f, t.n);
  t.nw = __fmul_rn(t.s, t.e); t.ne = __fmul_rn(t.s, t.w);
  t.sw = __fmul_rn(t.n, t.e); t.se = __fmul_rn(t.n, t.w);
  // floor of a possibly huge/NaN coordinate: clamp before the int conversion
  const float cx = fminf(fmaxf(fx, -2.f), (float)W + 1.f), cy = fminf(fmaxf(fy, -2.f), (float)H + 1.f);
  t.x0 = (int)cx; t.y0 = (int)cy;
  t.okx0 = (t.x0 >= 0) & (t.x0 < W); t.okx1 = (t.x0 + 1 >= 0) & (t.x0 + 1 < W);
  t.oky0 = (t.y0 >= 0) & (t.y0 < H); t.oky1 = (t.y0 + 1 >= 0) & (t.y0 + 1 < H);
  return t;
}
// the chain over the four taps' values (0 for a tap outside the plane)
__device__ __forceinline__ float sample_chain(float vnw, float vne, float vsw, float vse, const Taps& t) {
  float acc = __fmul_rn(vnw, t.nw);
  acc = __fmaf_rn(vne, t.ne, acc);
  acc = __fmaf_rn(vsw, t.sw, acc);
  acc = __fmaf_rn(vse, t.se, acc);
  return acc;
}
__device__ __forceinline__ float sample_plane(const float* __restrict__ p, int W, const Taps& t) {
  const float vnw = (t.oky0 & t.okx0) ? p[(long)t.y0 * W + t.x0] : 0.f;
  const float vne = (t.oky0 & t.okx1) ? p[(long)t.y0 * W + t.x0 + 1] : 0.f;
  const float vsw = (t.oky1 & t.okx0) ? p[(long)(t.y0 + 1) * W + t.x0] : 0.f;
  const float vse = (t.oky1 & t.okx1) ? p[(long)(t.y0 + 1) * W + t.x0 + 1] : 0.f;
  return sample_chain(vnw, vne, vsw, vse, t);
}

}  // namespace
