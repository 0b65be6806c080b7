// A frame a pass can read.  A (B,3,H,W) frame comes in four layouts, and every pass that takes one (gaze_gate.hip: tiles, commit;
// gaze_motion.hip: profiles, move; frames_u8.hip: the network's front; frame_overlay.hip) is written once, over a reader of the layout:
//   PlanarFrame<float>           fp32, the value of channel c at (b, y, x) is p[(b * 3 + c) * H * W + y * W + x]; its code is q(value)
//   PlanarFrame<unsigned char>   bytes in the same order; the pixel value is byte / 255, whose code is the byte
//   HwcFrame<SX>                 interleaved bytes read where they lie (fs_*_hwc; include/fovealseg.h "frames as interleaved bytes"): the
//                                byte of channel c at (b, y, x) is p[b * sb + y * sy + x * sx + c], sx = 3 (RGB) or 4 (RGBA / RGBX, the
//                                fourth byte never read into a result), rows of any pitch sy >= W * sx, images sb apart or all one image
//                                (sb = 0).  SX = 3 or 4 where the pass knows the step at compile time (the vector forms), 0 for the sx
//                                given at run time (the one-pixel forms).
//   Nv12Frame                    a decoder's surface read where it lies (fs_*_nv12; include/fovealseg.h "frames as NV12"): a luma plane and a
//                                plane of interleaved chroma at half the resolution; the pixel's RGB byte, a fixed integer function of
//                                (Y, U, V), is its code.  A pixel's position is an Nv12Px, not one pointer: the passes hold it as `auto`.
// A reader is built inside the kernel from the kernel's own pointer and scalars, and on the host from an entry point's arguments.  On the
// device it offers the few reads the passes use, all from a pixel's address px(b, y, x): the code of a channel, the luma codes of four
// pixels from aligned loads, sixteen bytes a channel in planar order (bytes only), and a tap's value (float)byte / 255, correctly rounded
// (bytes only).  On the host it carries what it accepts (ok), when its vector forms apply (wide, quad, wide_commit) and how many key
// bytes a lane of commit's vector form writes (lane).
#pragma once
#include "common.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The pixel code q(v) = (int) rintf(fminf(fmaxf(v, 0), 1) * 255.0f): one fp32 multiply, round to nearest even; NaN -> 0.  The clamps are
// written as comparisons so that a NaN takes the first branch's 0 whatever the min / max instructions make of it.  One function for every
// pass: a frame against the key that commit made from it differs nowhere, NaN pixels included.
__device__ __forceinline__ int pixel_q(float v) {
  v = v > 0.f ? v : 0.f;
  v = v < 1.f ? v : 1.f;
  return (int)rintf(__fmul_rn(v, 255.0f));
}
__device__ __forceinline__ int pixel_q(unsigned char v) { return (int)v; }

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

// The inverses, for a pass that writes a frame (frame_overlay.hip): one dword a channel, pixel j in byte j -> four pixels of interleaved
// bytes.  RGB: d0 = r0 g0 b0 r1, d1 = g1 b1 r2 g2, d2 = b2 r3 g3 b3; R and G meet first, B fills its bytes: two perms a dword.
__device__ __forceinline__ void hwc_join3(unsigned int r, unsigned int g, unsigned int b, unsigned int& d0, unsigned int& d1,
                                          unsigned int& d2) {
  d0 = hwc_perm(b, hwc_perm(g, r, hwc_sel(0, 4, 0, 1)), hwc_sel(0, 1, 4, 3));
  d1 = hwc_perm(b, hwc_perm(g, r, hwc_sel(5, 0, 2, 6)), hwc_sel(0, 5, 2, 3));
  d2 = hwc_perm(b, hwc_perm(g, r, hwc_sel(0, 3, 7, 0)), hwc_sel(6, 1, 2, 7));
}
// RGBA: a dword a pixel, its fourth byte 255.  R G pairs and B 255 pairs, then a pixel from each: eight perms.
__device__ __forceinline__ void hwc_join4(unsigned int r, unsigned int g, unsigned int b, unsigned int& d0, unsigned int& d1,
                                          unsigned int& d2, unsigned int& d3) {
  const unsigned int u0 = hwc_perm(g, r, hwc_sel(0, 4, 1, 5)), u1 = hwc_perm(g, r, hwc_sel(2, 6, 3, 7));          // R G R G
  const unsigned int v0 = hwc_perm(0xffffffffu, b, hwc_sel(0, 4, 1, 4)), v1 = hwc_perm(0xffffffffu, b, hwc_sel(2, 4, 3, 4));      // B 255 B 255
  d0 = hwc_perm(v0, u0, hwc_sel(0, 1, 4, 5));
  d1 = hwc_perm(v0, u0, hwc_sel(2, 3, 6, 7));
  d2 = hwc_perm(v1, u1, hwc_sel(0, 1, 4, 5));
  d3 = hwc_perm(v1, u1, hwc_sel(2, 3, 6, 7));
}

// Four codes from one aligned load, added to l: 16 bytes of fp32, 4 of bytes.
__device__ __forceinline__ void code4(const float* p, int* l) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(p);
  l[0] += pixel_q(v.x), l[1] += pixel_q(v.y), l[2] += pixel_q(v.z), l[3] += pixel_q(v.w);
}
__device__ __forceinline__ void code4(const unsigned char* p, int* l) {
  const unsigned int k = *reinterpret_cast<const unsigned int*>(p);
  l[0] += (int)(k & 255u), l[1] += (int)((k >> 8) & 255u), l[2] += (int)((k >> 16) & 255u), l[3] += (int)(k >> 24);
}

template <typename T>
struct PlanarFrame {
  static constexpr int lane = sizeof(T) == 4 ? 4 : 16;           // commit's vector form: four codes of a 16-byte load, or sixteen bytes
  const T* p;
  size_t plane;
  int W;
  __host__ __device__ PlanarFrame(const T* p_, int H, int W_) : p(p_), plane((size_t)H * W_), W(W_) {}

  __device__ __forceinline__ const T* px(size_t b, int y, int x) const { return p + b * 3 * plane + (size_t)y * W + x; }
  __device__ __forceinline__ const T* down(const T* a, int rows) const { return a + (size_t)rows * W; }
  __device__ __forceinline__ const T* right(const T* a, int cols) const { return a + cols; }
  __device__ __forceinline__ int code(const T* a, int c) const { return pixel_q(a[c * plane]); }
  // the code of element e = (c, y, x) of viewer b's frame in the key's order, which is this frame's own: e alone is used
  __device__ __forceinline__ int code_of(size_t b, size_t e, int, int, int) const { return pixel_q(p[b * 3 * plane + e]); }
  __device__ __forceinline__ void luma4(const T* a, int* l) const {      // l[j] += the three codes of pixel j, j < 4
#pragma unroll
    for (int c = 0; c < 3; ++c) code4(a + c * plane, l);
  }
  __device__ __forceinline__ void load16(const T* a, u32x4* v) const {   // bytes: v[c] = sixteen pixels of channel c
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const u32x4*>(a + c * plane);
  }
  __device__ __forceinline__ float tap(const T* a, int c) const { return __fdiv_rn((float)a[c * plane], 255.0f); }

  explicit operator bool() const { return p != nullptr; }
  bool ok(int, int, int) const { return true; }
  // every lane-pixel piece of every row is one aligned load (the tile pass, commit)
  bool wide(int W_) const { return W_ % lane == 0 && ((uintptr_t)p & 15) == 0; }
  // commit copies a planar frame of bytes as one run: whole 16-byte pieces a viewer, wherever the rows end
  bool wide_commit(int W_, size_t per) const { return sizeof(T) == 4 ? wide(W_) : per % 16 == 0 && ((uintptr_t)p & 15) == 0; }
  // every four-pixel piece of every row is one aligned load (the profile pass)
  bool quad(int W_) const { return W_ % 4 == 0 && ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0; }
};

template <int SX>
struct HwcFrame {
  static constexpr int lane = 48;                                 // commit's vector form: sixteen pixels, sixteen bytes a channel
  const unsigned char* p;
  long sb, sy;
  int sx;
  __host__ __device__ HwcFrame(const unsigned char* p_, long sb_, long sy_, int sx_) : p(p_), sb(sb_), sy(sy_), sx(sx_) {}

  __device__ __forceinline__ int step() const { return SX > 0 ? SX : sx; }
  __device__ __forceinline__ const unsigned char* px(size_t b, int y, int x) const {
    return p + b * (size_t)sb + (size_t)y * sy + (size_t)x * step();
  }
  __device__ __forceinline__ const unsigned char* down(const unsigned char* a, int rows) const { return a + (size_t)rows * sy; }
  __device__ __forceinline__ const unsigned char* right(const unsigned char* a, int cols) const { return a + (size_t)cols * step(); }
  __device__ __forceinline__ int code(const unsigned char* a, int c) const { return (int)a[c]; }
  __device__ __forceinline__ int code_of(size_t b, size_t, int c, int y, int x) const { return (int)px(b, y, x)[c]; }     // (c, y, x) are used
  // Four pixels are 12 bytes in three 4-byte loads (SX = 3) or one 16-byte load (SX = 4); a pixel's luma is the sum of its three bytes
  // (v_sad_u8 against 0), the fourth byte of an RGBA pixel masked off.  Added to l, as the planar frames' are.
  __device__ __forceinline__ void luma4(const unsigned char* a, int* l) const {
    if (SX == 3) {
      const unsigned int w0 = *reinterpret_cast<const unsigned int*>(a), w1 = *reinterpret_cast<const unsigned int*>(a + 4),
                         w2 = *reinterpret_cast<const unsigned int*>(a + 8);
      l[0] += (int)__builtin_amdgcn_sad_u8(w0 & 0x00ffffffu, 0u, 0u);
      l[1] += (int)__builtin_amdgcn_sad_u8(w0 >> 24, 0u, __builtin_amdgcn_sad_u8(w1 & 0x0000ffffu, 0u, 0u));
      l[2] += (int)__builtin_amdgcn_sad_u8(w1 >> 16, 0u, __builtin_amdgcn_sad_u8(w2 & 0x000000ffu, 0u, 0u));
      l[3] += (int)__builtin_amdgcn_sad_u8(w2 >> 8, 0u, 0u);
    } else {
      const u32x4 v = *reinterpret_cast<const u32x4*>(a);
      l[0] += (int)__builtin_amdgcn_sad_u8(v.x & 0x00ffffffu, 0u, 0u);
      l[1] += (int)__builtin_amdgcn_sad_u8(v.y & 0x00ffffffu, 0u, 0u);
      l[2] += (int)__builtin_amdgcn_sad_u8(v.z & 0x00ffffffu, 0u, 0u);
      l[3] += (int)__builtin_amdgcn_sad_u8(v.w & 0x00ffffffu, 0u, 0u);
    }
  }
  // Sixteen pixels of a row from their 48 (SX = 3) or 64 (SX = 4) bytes, 16-byte aligned: three or four 16-byte loads, then v[c] = the
  // sixteen bytes of channel c in planar order.
  __device__ __forceinline__ void load16(const unsigned char* __restrict__ a, u32x4* v) const {
    const u32x4* q = reinterpret_cast<const u32x4*>(a);
    unsigned int o[3][4];
    if (SX == 3) {
      const u32x4 a0 = q[0], a1 = q[1], a2 = q[2];
      hwc_split3(a0.x, a0.y, a0.z, o[0][0], o[1][0], o[2][0]);
      hwc_split3(a0.w, a1.x, a1.y, o[0][1], o[1][1], o[2][1]);
      hwc_split3(a1.z, a1.w, a2.x, o[0][2], o[1][2], o[2][2]);
      hwc_split3(a2.y, a2.z, a2.w, o[0][3], o[1][3], o[2][3]);
    } else {
      const u32x4 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3];
      hwc_split4(a0.x, a0.y, a0.z, a0.w, o[0][0], o[1][0], o[2][0]);
      hwc_split4(a1.x, a1.y, a1.z, a1.w, o[0][1], o[1][1], o[2][1]);
      hwc_split4(a2.x, a2.y, a2.z, a2.w, o[0][2], o[1][2], o[2][2]);
      hwc_split4(a3.x, a3.y, a3.z, a3.w, o[0][3], o[1][3], o[2][3]);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) v[ch] = u32x4{o[ch][0], o[ch][1], o[ch][2], o[ch][3]};
  }
  __device__ __forceinline__ float tap(const unsigned char* a, int c) const { return __fdiv_rn((float)a[c], 255.0f); }

  explicit operator bool() const { return p != nullptr; }
  // a row of W pixels can be read: the pointer, the pixel step, the pitch and the image step
  bool row_ok(int W) const { return p != nullptr && (sx == 3 || sx == 4) && W > 0 && sy >= (long)W * sx && sb >= 0; }
  // what every fs_*_hwc entry point asks of the description beyond its twin's conditions: rows, and images that do not overlap
  bool ok(int B, int H, int W) const { return row_ok(W) && H > 0 && !(B > 1 && sb > 0 && sb < (long)H * sy); }
  // fs_byte_frame_route: -1 no readable row, 1 the vector forms (sixteen pixels a lane of the tile and commit passes, four of the profile
  // pass: every 16-pixel piece of every row starts at a multiple of 16 bytes), 0 the one-pixel forms
  long route(int W) const {
    if (!row_ok(W)) return -1;
    return (W % 16 == 0 && ((uintptr_t)p & 15) == 0 && sy % 16 == 0 && sb % 16 == 0) ? 1 : 0;
  }
  bool wide(int W) const { return route(W) == 1; }
  bool wide_commit(int W, size_t) const { return wide(W); }
  bool quad(int W) const { return wide(W); }
};

// An NV12 frame, as a video decoder or a camera makes it (fs_*_nv12; include/fovealseg.h "frames as NV12"): a plane of luma bytes, Y of
// (b, y, x) = yp[b * sb + y * sy + x], and a plane of interleaved chroma at half the resolution both ways, (U, V) of (b, y, x) = uvp[b * ub +
// (y >> 1) * uy + 2 * (x >> 1) + (0, 1)]: the sample of the pixel's 2 x 2 block, replicated.  Rows of any pitch sy >= W, uy >= 2 * ceil(W /
// 2); images apart or all one image (sb = ub = 0).  The RGB byte of a pixel is a fixed integer function of (Y, U, V) and the table csc
// (nv12_rgb below), that byte is the pixel's code and byte / 255 its value: every pass gives on an NV12 frame what it gives on the planar
// frame of those bytes, bit for bit.
struct Nv12Csc {
  int yo, yg, rv, gu, gv, bu;
  // no sum of nv12_rgb leaves int32: |yg * C| + 2 * 32768 * 128 + 128 < 2^25
  bool ok() const {
    const int co[5] = {yg, rv, gu, gv, bu};
    for (int c : co)
      if (c < -32768 || c > 32768) return false;
    return yo >= 0 && yo <= 255;
  }
};
// A pixel's position: where its luma byte and its chroma pair lie, and the parities of its column (bit 0) and row (bit 1), which say
// when a step right or down reaches the next chroma sample.
struct Nv12Px {
  const unsigned char* lu;
  const unsigned char* ch;
  int par;
};

// the chroma products of one sample, made once for the two or four pixels that share it
struct Nv12Chroma {
  int r, g, b;
};
__device__ __forceinline__ Nv12Chroma nv12_chroma(const Nv12Csc& k, int U, int V) {
  const int D = U - 128, E = V - 128;
  return Nv12Chroma{k.rv * E, k.gu * D + k.gv * E, k.bu * D};
}
// clamp(v >> 8, 0, 255), written as the clamp first and the shift after it: v < 0 -> 0, v >= 65536 -> 65535 >> 8 = 255, v >> 8 between.
// Spelled the other way round, two neighbours OR-ed into one word are selected as v_ashr_pk_u8_i32 (gfx950), whose result the compiler
// takes to have sixteen zero bits on top; on the hardware the pixels above a negative sum then read 255 (profiles/r35/README.md).
// Do not simplify it back.  Nothing but the compiler's choice keeps that instruction away from this spelling: after a change of
// toolchain, test_nv12_to_rgb_over_all_triplets (tests/test_frames_nv12.py, on the GPU) is what says whether it still does.
__device__ __forceinline__ int nv12_clamp(int v) { return min(max(v, 0), 65535) >> 8; }
// R, G, B = clamp((yg * (Y - yo) + the channel's chroma product + 128) >> 8, 0, 255), >> the arithmetic shift
__device__ __forceinline__ void nv12_rgb(const Nv12Csc& k, int Y, const Nv12Chroma& m, int& r, int& g, int& b) {
  const int l = k.yg * (Y - k.yo) + 128;
  r = nv12_clamp(l + m.r), g = nv12_clamp(l + m.g), b = nv12_clamp(l + m.b);
}

struct Nv12Frame {
  static constexpr int lane = 48;                                 // commit's vector form: sixteen pixels, sixteen key bytes a channel
  const unsigned char* yp;
  const unsigned char* uvp;
  long sb, sy, ub, uy;
  Nv12Csc k;
  __host__ __device__ Nv12Frame(const unsigned char* yp_, const unsigned char* uvp_, long sb_, long sy_, long ub_, long uy_, const Nv12Csc& k_)
      : yp(yp_), uvp(uvp_), sb(sb_), sy(sy_), ub(ub_), uy(uy_), k(k_) {}

  // y >> 1 and x >> 1 are arithmetic: a position one step outside the frame (a tap never read) steps back into it by right / down
  __device__ __forceinline__ Nv12Px px(size_t b, int y, int x) const {
    return Nv12Px{yp + b * (size_t)sb + (long)y * sy + x, uvp + b * (size_t)ub + (long)(y >> 1) * uy + 2 * (long)(x >> 1), (x & 1) | ((y & 1) << 1)};
  }
  __device__ __forceinline__ Nv12Px down(const Nv12Px& a, int rows) const {                // rows >= 0
    const int n = (a.par >> 1) + rows;
    return Nv12Px{a.lu + (size_t)rows * sy, a.ch + (size_t)(n >> 1) * uy, (a.par & 1) | ((n & 1) << 1)};
  }
  __device__ __forceinline__ Nv12Px right(const Nv12Px& a, int cols) const {               // cols >= 0
    const int n = (a.par & 1) + cols;
    return Nv12Px{a.lu + cols, a.ch + 2 * (size_t)(n >> 1), (a.par & 2) | (n & 1)};
  }
  __device__ __forceinline__ int code(const Nv12Px& a, int c) const {
    int r, g, bl;
    nv12_rgb(k, (int)a.lu[0], nv12_chroma(k, (int)a.ch[0], (int)a.ch[1]), r, g, bl);
    return c == 0 ? r : c == 1 ? g : bl;
  }
  __device__ __forceinline__ int code_of(size_t b, size_t, int c, int y, int x) const { return code(px(b, y, x), c); }       // (c, y, x) are used
  // Four pixels of a row, x a multiple of 4 and the vector form's alignment: 4 luma bytes and their two chroma pairs, a 4-byte load each
  __device__ __forceinline__ void luma4(const Nv12Px& a, int* l) const {
    const unsigned int y4 = *reinterpret_cast<const unsigned int*>(a.lu), c4 = *reinterpret_cast<const unsigned int*>(a.ch);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const Nv12Chroma m = nv12_chroma(k, (int)((c4 >> (16 * p)) & 255u), (int)((c4 >> (16 * p + 8)) & 255u));
#pragma unroll
      for (int j = 2 * p; j < 2 * p + 2; ++j) {
        int r, g, bl;
        nv12_rgb(k, (int)((y4 >> (8 * j)) & 255u), m, r, g, bl);
        l[j] += r + g + bl;
      }
    }
  }
  // Sixteen pixels of a row, x a multiple of 16 and the vector form's alignment: one 16-byte load of luma and one of chroma, its eight
  // samples' products made once each; v[c] = the sixteen bytes of channel c in planar order
  __device__ __forceinline__ void load16(const Nv12Px& a, u32x4* v) const {
    const u32x4 y16 = *reinterpret_cast<const u32x4*>(a.lu), c16 = *reinterpret_cast<const u32x4*>(a.ch);
    const unsigned int yw[4] = {y16.x, y16.y, y16.z, y16.w}, cw[4] = {c16.x, c16.y, c16.z, c16.w};
    unsigned int o[3][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                       // luma word q: pixels 4q .. 4q + 3, the chroma pairs of word q
      unsigned int w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const Nv12Chroma m = nv12_chroma(k, (int)((cw[q] >> (16 * p)) & 255u), (int)((cw[q] >> (16 * p + 8)) & 255u));
#pragma unroll
        for (int j = 2 * p; j < 2 * p + 2; ++j) {
          int r, g, bl;
          nv12_rgb(k, (int)((yw[q] >> (8 * j)) & 255u), m, r, g, bl);
          w[0] |= (unsigned int)r << (8 * j), w[1] |= (unsigned int)g << (8 * j), w[2] |= (unsigned int)bl << (8 * j);
        }
      }
      o[0][q] = w[0], o[1][q] = w[1], o[2][q] = w[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = u32x4{o[c][0], o[c][1], o[c][2], o[c][3]};
  }
  __device__ __forceinline__ float tap(const Nv12Px& a, int c) const { return __fdiv_rn((float)code(a, c), 255.0f); }

  explicit operator bool() const { return yp != nullptr && uvp != nullptr; }
  // a row of W pixels and its chroma row can be read, and the table keeps every sum in int32
  bool row_ok(int W) const {
    return yp != nullptr && uvp != nullptr && W > 0 && sy >= (long)W && uy >= 2 * (((long)W + 1) / 2) && sb >= 0 && ub >= 0 && k.ok();
  }
  // what every fs_*_nv12 entry point asks of the description beyond its twin's conditions: rows, and images that do not overlap in either
  // plane or are all one image
  bool ok(int B, int H, int W) const {
    if (!row_ok(W) || H <= 0) return false;
    if (B <= 1 || (sb == 0 && ub == 0)) return true;
    return sb >= (long)H * sy && ub >= (((long)H + 1) / 2) * uy;
  }
  // fs_nv12_frame_route: -1 no readable row, 1 the vector forms (every 16-pixel piece of every luma row and its 16 chroma bytes start at
  // a multiple of 16 bytes), 0 the one-pixel forms
  long route(int W) const {
    if (!row_ok(W)) return -1;
    return (W % 16 == 0 && (((uintptr_t)yp | (uintptr_t)uvp) & 15) == 0 && sy % 16 == 0 && sb % 16 == 0 && uy % 16 == 0 && ub % 16 == 0) ? 1 : 0;
  }
  bool wide(int W) const { return route(W) == 1; }
  bool wide_commit(int W, size_t) const { return wide(W); }
  bool quad(int W) const { return wide(W); }
};

// A frame a pass can write (frame_overlay.hip): always bytes, described by (p, ob, oy, ox).  ox = 1, planar: the byte of channel c at
// (b, y, x) is p[b * ob + c * H * W + y * W + x], oy == W, images ob >= 3 * H * W apart.  ox = 3 or 4, interleaved: p[b * ob + y * oy + x *
// ox + c], rows of any pitch oy >= W * ox, images ob >= H * oy apart; the fourth byte of an RGBA pixel is written as 255.  OX = 1, 3 or 4
// where the pass knows the step at compile time (the vector forms), 0 for the ox given at run time (the one-pixel forms).  A pixel is
// stored as three or four bytes, sixteen pixels of a row -- sixteen bytes a channel in planar order, what a reader's load16 gives -- as
// three or four 16-byte pieces: stored by their lane (store16), or joined (join16) for a pass that lets other lanes store them (piece).
template <int OX>
struct FrameWriter {
  unsigned char* p;
  long ob, oy;
  int ox;
  size_t plane;
  __host__ __device__ FrameWriter(unsigned char* p_, long ob_, long oy_, int ox_, int H, int W) : p(p_), ob(ob_), oy(oy_), ox(ox_), plane((size_t)H * W) {}

  __device__ __forceinline__ int step() const { return OX > 0 ? OX : ox; }
  __device__ __forceinline__ void store1(size_t b, int y, int x, int r, int g, int bl) const {
    if (step() == 1) {
      unsigned char* a = p + b * (size_t)ob + (size_t)y * oy + x;
      a[0] = (unsigned char)r, a[plane] = (unsigned char)g, a[2 * plane] = (unsigned char)bl;
    } else {
      unsigned char* a = p + b * (size_t)ob + (size_t)y * oy + (size_t)x * step();
      a[0] = (unsigned char)r, a[1] = (unsigned char)g, a[2] = (unsigned char)bl;
      if (step() == 4) a[3] = 255;
    }
  }
  // where pixel (b, y, x) of an interleaved destination begins (channel 0 of a planar one)
  __device__ __forceinline__ unsigned char* piece(size_t b, int y, int x) const { return p + b * (size_t)ob + (size_t)y * oy + (size_t)x * step(); }
  // Sixteen pixels, v[c][q] = pixels 4q .. 4q + 3 of channel c, pixel j in byte j, as the OX = 3 or 4 16-byte pieces they are in memory
  __device__ __forceinline__ void join16(const unsigned int (*v)[4], u32x4* m) const {
    if (OX == 3) {
      unsigned int d[12];
#pragma unroll
      for (int q = 0; q < 4; ++q) hwc_join3(v[0][q], v[1][q], v[2][q], d[3 * q], d[3 * q + 1], d[3 * q + 2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) m[i] = u32x4{d[4 * i], d[4 * i + 1], d[4 * i + 2], d[4 * i + 3]};
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        unsigned int d0, d1, d2, d3;
        hwc_join4(v[0][q], v[1][q], v[2][q], d0, d1, d2, d3);
        m[q] = u32x4{d0, d1, d2, d3};
      }
    }
  }
  // the sixteen pixels stored by their own lane; x a multiple of 16 and the address 16-byte aligned (wide)
  __device__ __forceinline__ void store16(size_t b, int y, int x, const unsigned int (*v)[4]) const {
    if (OX == 1) {
      unsigned char* a = piece(b, y, x);
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<u32x4*>(a + c * plane) = u32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
    } else {
      u32x4 m[OX > 1 ? OX : 1];
      join16(v, m);
      u32x4* a = reinterpret_cast<u32x4*>(piece(b, y, x));
#pragma unroll
      for (int i = 0; i < OX; ++i) a[i] = m[i];
    }
  }

  // the description can be written: the pointer, the pixel step, the pitch and an image step that keeps B images apart
  bool ok(int B, int H, int W) const {
    if (p == nullptr || B < 1 || H < 1 || W < 1 || ob < 0) return false;
    if (ox == 1) return oy == W && (B == 1 || ob >= 3 * (long)H * W);
    return (ox == 3 || ox == 4) && oy >= (long)W * ox && (B == 1 || ob >= (long)H * oy);
  }
  // every 16-pixel piece of every row (and plane) starts at a multiple of 16 bytes: HwcFrame::route's conditions, or aligned planes
  bool wide(int W) const { return W % 16 == 0 && ((uintptr_t)p & 15) == 0 && oy % 16 == 0 && ob % 16 == 0; }
};

}  // namespace
