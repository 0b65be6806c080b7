// A frame of interleaved bytes read where it lies (fs_*_hwc; include/fovealseg.h "frames as interleaved bytes"): the byte of channel c at
// (b, y, x) is p[b * sb + y * sy + x * sx + c], sx = 3 (RGB) or 4 (RGBA / RGBX, the fourth byte never read into a result), rows of any
// pitch sy >= W * sx, images sb apart or all one image (sb = 0).  One description, one acceptance rule and one choice of route for
// every pass that takes such a frame: frames_u8.hip (the network's front), gaze_gate.hip (tiles, commit), gaze_motion.hip (profiles, move).
#pragma once
#include "common.h"

typedef unsigned int hwc_u32x4 __attribute__((ext_vector_type(4)));

struct HwcView {
  const unsigned char* p;
  long sb, sy;
  int sx;
  explicit operator bool() const { return p != nullptr; }
};

// what every fs_*_hwc entry point asks of the description beyond its twin's conditions
inline bool hwc_view_ok(const HwcView& v, int B, int H, int W) {
  if (v.p == nullptr || (v.sx != 3 && v.sx != 4) || W <= 0 || H <= 0 || v.sy < (long)W * v.sx || v.sb < 0) return false;
  return !(B > 1 && v.sb > 0 && v.sb < (long)H * v.sy);      // images that overlap
}

// fs_byte_frame_route: -1 refused, 1 the vector forms (sixteen pixels a lane of the tile and commit passes, four of the profile pass:
// every 16-pixel piece of every row starts at a multiple of 16 bytes), 0 the one-pixel forms
inline long hwc_route(const unsigned char* p, long sb, long sy, int sx, int W) {
  if (p == nullptr || (sx != 3 && sx != 4) || W <= 0 || sy < (long)W * sx || sb < 0) return -1;
  return (W % 16 == 0 && ((uintptr_t)p & 15) == 0 && sy % 16 == 0 && sb % 16 == 0) ? 1 : 0;
}
inline bool hwc_vec_ok(const HwcView& v, int W) { return hwc_route(v.p, v.sb, v.sy, v.sx, W) == 1; }

#if defined(__HIPCC__)
namespace {

constexpr unsigned int hwc_sel(unsigned int b0, unsigned int b1, unsigned int b2, unsigned int b3) {
  return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}
// v_perm_b32: result byte i = byte sel[i] of the eight bytes {lo: 0..3, hi: 4..7}
__device__ __forceinline__ unsigned int hwc_perm(unsigned int hi, unsigned int lo, unsigned int sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// Four pixels of interleaved bytes -> one dword a channel, pixel j in byte j (the order of a planar row).
// RGB: 12 bytes d0 d1 d2, channel c at bytes c, c + 3, c + 6, c + 9: two perms a channel.
__device__ __forceinline__ void hwc_split3(unsigned int d0, unsigned int d1, unsigned int d2, unsigned int& r, unsigned int& g,
                                           unsigned int& b) {
  r = hwc_perm(d2, hwc_perm(d1, d0, hwc_sel(0, 3, 6, 0)), hwc_sel(0, 1, 2, 5));
  g = hwc_perm(d2, hwc_perm(d1, d0, hwc_sel(1, 4, 7, 0)), hwc_sel(0, 1, 2, 6));
  b = hwc_perm(d2, hwc_perm(d1, d0, hwc_sel(2, 5, 0, 0)), hwc_sel(0, 1, 4, 7));
}
// RGBA: a dword a pixel.  R and G share their first step, seven perms in all; byte 3 of a pixel is selected by none of them.
__device__ __forceinline__ void hwc_split4(unsigned int d0, unsigned int d1, unsigned int d2, unsigned int d3, unsigned int& r,
                                           unsigned int& g, unsigned int& b) {
  const unsigned int u0 = hwc_perm(d1, d0, hwc_sel(0, 4, 1, 5)), u1 = hwc_perm(d3, d2, hwc_sel(0, 4, 1, 5));      // R R G G
  const unsigned int v0 = hwc_perm(d1, d0, hwc_sel(2, 6, 2, 6)), v1 = hwc_perm(d3, d2, hwc_sel(2, 6, 2, 6));      // B B B B
  r = hwc_perm(u1, u0, hwc_sel(0, 1, 4, 5));
  g = hwc_perm(u1, u0, hwc_sel(2, 3, 6, 7));
  b = hwc_perm(v1, v0, hwc_sel(0, 1, 4, 5));
}

// Sixteen pixels of a row from their 48 (SX = 3) or 64 (SX = 4) bytes, 16-byte aligned: three or four 16-byte loads, then v[c] =
// the sixteen bytes of channel c in planar order.
template <int SX>
__device__ __forceinline__ void hwc_load16(const unsigned char* __restrict__ p, hwc_u32x4* v) {
  const hwc_u32x4* q = reinterpret_cast<const hwc_u32x4*>(p);
  unsigned int o[3][4];
  if (SX == 3) {
    const hwc_u32x4 a = q[0], b = q[1], c = q[2];
    hwc_split3(a.x, a.y, a.z, o[0][0], o[1][0], o[2][0]);
    hwc_split3(a.w, b.x, b.y, o[0][1], o[1][1], o[2][1]);
    hwc_split3(b.z, b.w, c.x, o[0][2], o[1][2], o[2][2]);
    hwc_split3(c.y, c.z, c.w, o[0][3], o[1][3], o[2][3]);
  } else {
    const hwc_u32x4 a = q[0], b = q[1], c = q[2], d = q[3];
    hwc_split4(a.x, a.y, a.z, a.w, o[0][0], o[1][0], o[2][0]);
    hwc_split4(b.x, b.y, b.z, b.w, o[0][1], o[1][1], o[2][1]);
    hwc_split4(c.x, c.y, c.z, c.w, o[0][2], o[1][2], o[2][2]);
    hwc_split4(d.x, d.y, d.z, d.w, o[0][3], o[1][3], o[2][3]);
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) v[ch] = hwc_u32x4{o[ch][0], o[ch][1], o[ch][2], o[ch][3]};
}

}  // namespace
#endif
