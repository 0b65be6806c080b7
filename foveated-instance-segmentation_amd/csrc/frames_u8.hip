// The network's front for a frame of bytes: a planar (B,3,H,W) uint8 frame whose pixel value is v = (float)byte / 255.0f, correctly
// rounded -- ingest_sample_kernel's expression (frontend.hip).  The network reads the frame through two gathers only, four taps a
// point each, so no fp32 frame needs to exist: the taps are converted as they are read and everything after the conversion is the fp32
// kernel's arithmetic, bit for bit.  The gate and the motion passes of such a frame are in gaze_gate.hip and gaze_motion.hip.
//   gaze_lowres_u8_kernel   K1 of frontend.hip on bytes (fs_gaze_lowres_u8_fwd)
//   grid_sample_u8_kernel   K5 of frontend.hip on bytes, forward only (fs_grid_sample_u8_fwd)
// The same two gathers read an interleaved frame where it lies (frame_view.h: the byte of channel c at (b, y, x) is x[b * sb + y * sy +
// x * sx + c]); a tap's three bytes are neighbours, so a tap is one address.  Their bodies are spelled out beside the planar ones.
//   gaze_lowres_hwc_kernel  fs_gaze_lowres_hwc_fwd
//   grid_sample_hwc_kernel  fs_grid_sample_hwc_fwd (three channels)
#include "common.h"
#include "frame_view.h"
#include "grid_taps.h"

namespace {

__device__ __forceinline__ float u8_value(unsigned char b) { return __fdiv_rn((float)b, 255.0f); }

// gaze_lowres_kernel with the four taps converted.  Where that kernel leaves an expression to the compiler's contraction, this one spells
// the operations its code performs, so that the two stay equal bit for bit whatever the optimiser makes of the conversions around them:
// contraction is off for the whole body, whose sums and products are plain operators, and every fused multiply-add is an explicit
// __fmaf_rn.  (HIP's __fadd_rn / __fmul_rn are inline functions of plain operators compiled under -ffp-contract=fast: the pragma does
// not reach into them, and a sum of their products is still fused.)
__global__ __launch_bounds__(256) void gaze_lowres_u8_kernel(const unsigned char* __restrict__ x, const float* __restrict__ focus,
                                                             float* __restrict__ out, int B, int H, int W, int hs, int ws) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * hs * ws) return;
  const int ox = (int)(i % ws), oy = (int)((i / ws) % hs), b = (int)(i / ((long)ws * hs));
  const float sy = (float)H / (float)hs, sx = (float)W / (float)ws;
  float fy = __fmaf_rn(sy, (float)oy + 0.5f, -0.5f); if (fy < 0.f) fy = 0.f;
  float fx = __fmaf_rn(sx, (float)ox + 0.5f, -0.5f); if (fx < 0.f) fx = 0.f;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float ly1 = fy - (float)y0, ly0 = 1.f - ly1, lx1 = fx - (float)x0, lx0 = 1.f - lx1;
  float* o = out + i * 5;
  // gaze_lowres_kernel leaves  ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)  to the compiler's contraction, and its
  // code (-O3, gfx950) came out differently per channel: the rows of channels 0 and 1 are r0 = fma(lx1, v01, lx0 * v00) and r1 =
  // fma(lx0, v10, lx1 * v11), channel 0 ends in fma(ly1, r1, ly0 * r0), channel 1 in fma(ly0, r0, ly1 * r1), and channel 2, whose
  // products were packed two a register, fuses nothing.  Spelled here operation for operation (profiles/r27/README.md); the test
  // against the fp32 kernel at the C ABI holds the two together.
  float v[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned char* p = x + ((long)b * 3 + c) * H * W;
    v[c][0] = u8_value(p[(long)y0 * W + x0]), v[c][1] = u8_value(p[(long)y0 * W + x1]);
    v[c][2] = u8_value(p[(long)y1 * W + x0]), v[c][3] = u8_value(p[(long)y1 * W + x1]);
  }
  {
    const float r0 = __fmaf_rn(lx1, v[0][1], lx0 * v[0][0]), r1 = __fmaf_rn(lx0, v[0][2], lx1 * v[0][3]);
    o[0] = __fmaf_rn(ly1, r1, ly0 * r0);
  }
  {
    const float r0 = __fmaf_rn(lx1, v[1][1], lx0 * v[1][0]), r1 = __fmaf_rn(lx0, v[1][2], lx1 * v[1][3]);
    o[1] = __fmaf_rn(ly0, r0, ly1 * r1);
  }
  {
    const float r0 = lx0 * v[2][0] + lx1 * v[2][1], r1 = lx0 * v[2][2] + lx1 * v[2][3];
    o[2] = ly0 * r0 + ly1 * r1;
  }
  // the gaze map: there (float)oy - focus * (hs - 1) is one fused multiply-add, the sum of the squares is not fused
  const float dy = __fmaf_rn(-focus[2 * b], (float)(hs - 1), (float)oy), dx = __fmaf_rn(-focus[2 * b + 1], (float)(ws - 1), (float)ox);
  const float dist = sqrtf(dy * dy + dx * dx);
  const float maxd = (float)sqrt((double)hs * hs + (double)ws * ws);
  const float r = dist / maxd;
  o[3] = r * r;
  o[4] = r * r;
}

// x (B,C,H,W) bytes -> out (B,h,w,C) NHWC [nhwc_out=1] or (B,C,h,w) NCHW [nhwc_out=0], fp32
__global__ __launch_bounds__(256) void grid_sample_u8_kernel(const unsigned char* __restrict__ x, const float* __restrict__ grid,
                                                             float* __restrict__ out, int B, int C, int H, int W, int h, int w, int nhwc_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * h * w) return;
  const int b = (int)(i / ((long)h * w));
  const long pix = i - (long)b * h * w;
  const Taps t = make_taps(grid[2 * i], grid[2 * i + 1], H, W);
  for (int c = 0; c < C; ++c) {
    const float v = sample_plane(x + ((long)b * C + c) * H * W, W, t);
    if (nhwc_out) out[i * C + c] = v;
    else out[((long)b * C + c) * h * w + pix] = v;
  }
}

// gaze_lowres_u8_kernel on an interleaved frame: the same four taps, the same operations in the same per-channel spelling.
__global__ __launch_bounds__(256) void gaze_lowres_hwc_kernel(const unsigned char* __restrict__ x, long sb, long sy, int sx,
                                                              const float* __restrict__ focus, float* __restrict__ out, int B, int H, int W,
                                                              int hs, int ws) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * hs * ws) return;
  const int ox = (int)(i % ws), oy = (int)((i / ws) % hs), b = (int)(i / ((long)ws * hs));
  const float scy = (float)H / (float)hs, scx = (float)W / (float)ws;
  float fy = __fmaf_rn(scy, (float)oy + 0.5f, -0.5f); if (fy < 0.f) fy = 0.f;
  float fx = __fmaf_rn(scx, (float)ox + 0.5f, -0.5f); if (fx < 0.f) fx = 0.f;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float ly1 = fy - (float)y0, ly0 = 1.f - ly1, lx1 = fx - (float)x0, lx0 = 1.f - lx1;
  float* o = out + i * 5;
  const unsigned char* p = x + (long)b * sb;
  const unsigned char* t00 = p + (long)y0 * sy + (long)x0 * sx;
  const unsigned char* t01 = p + (long)y0 * sy + (long)x1 * sx;
  const unsigned char* t10 = p + (long)y1 * sy + (long)x0 * sx;
  const unsigned char* t11 = p + (long)y1 * sy + (long)x1 * sx;
  float v[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[c][0] = u8_value(t00[c]), v[c][1] = u8_value(t01[c]);
    v[c][2] = u8_value(t10[c]), v[c][3] = u8_value(t11[c]);
  }
  {
    const float r0 = __fmaf_rn(lx1, v[0][1], lx0 * v[0][0]), r1 = __fmaf_rn(lx0, v[0][2], lx1 * v[0][3]);
    o[0] = __fmaf_rn(ly1, r1, ly0 * r0);
  }
  {
    const float r0 = __fmaf_rn(lx1, v[1][1], lx0 * v[1][0]), r1 = __fmaf_rn(lx0, v[1][2], lx1 * v[1][3]);
    o[1] = __fmaf_rn(ly0, r0, ly1 * r1);
  }
  {
    const float r0 = lx0 * v[2][0] + lx1 * v[2][1], r1 = lx0 * v[2][2] + lx1 * v[2][3];
    o[2] = ly0 * r0 + ly1 * r1;
  }
  const float dy = __fmaf_rn(-focus[2 * b], (float)(hs - 1), (float)oy), dx = __fmaf_rn(-focus[2 * b + 1], (float)(ws - 1), (float)ox);
  const float dist = sqrtf(dy * dy + dx * dx);
  const float maxd = (float)sqrt((double)hs * hs + (double)ws * ws);
  const float r = dist / maxd;
  o[3] = r * r;
  o[4] = r * r;
}

// grid_sample_u8_kernel on an interleaved frame of three channels: sample_plane's taps and chain, one address a tap
__global__ __launch_bounds__(256) void grid_sample_hwc_kernel(const unsigned char* __restrict__ x, long sb, long sy, int sx,
                                                              const float* __restrict__ grid, float* __restrict__ out, int B, int H, int W,
                                                              int h, int w, int nhwc_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * h * w) return;
  const int b = (int)(i / ((long)h * w));
  const long pix = i - (long)b * h * w;
  const Taps t = make_taps(grid[2 * i], grid[2 * i + 1], H, W);
  const unsigned char* p = x + (long)b * sb;
  const bool knw = t.oky0 & t.okx0, kne = t.oky0 & t.okx1, ksw = t.oky1 & t.okx0, kse = t.oky1 & t.okx1;
  const unsigned char* pnw = p + (long)t.y0 * sy + (long)t.x0 * sx;          // formed always, read only where the tap is inside
  const unsigned char* pne = pnw + sx;
  const unsigned char* psw = pnw + sy;
  const unsigned char* pse = psw + sx;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float vnw = knw ? __fdiv_rn((float)pnw[c], 255.0f) : 0.f;
    const float vne = kne ? __fdiv_rn((float)pne[c], 255.0f) : 0.f;
    const float vsw = ksw ? __fdiv_rn((float)psw[c], 255.0f) : 0.f;
    const float vse = kse ? __fdiv_rn((float)pse[c], 255.0f) : 0.f;
    float acc = __fmul_rn(vnw, t.nw);
    acc = __fmaf_rn(vne, t.ne, acc);
    acc = __fmaf_rn(vsw, t.sw, acc);
    acc = __fmaf_rn(vse, t.se, acc);
    if (nhwc_out) out[i * 3 + c] = acc;
    else out[((long)b * 3 + c) * h * w + pix] = acc;
  }
}

}  // namespace

extern "C" {

long fs_byte_frame_route(const unsigned char* img, long sb, long sy, int sx, int W) { return hwc_route(img, sb, sy, sx, W); }

int fs_gaze_lowres_hwc_fwd(const unsigned char* img, long sb, long sy, int sx, const float* focus, float* out, int B, int H, int W, int hs, int ws,
                           hipStream_t stream) {
  FS_REQUIRE(img && focus && out && B > 0 && H > 0 && W > 0 && hs > 1 && ws > 1 && hwc_view_ok(HwcView{img, sb, sy, sx}, B, H, W));
  hipLaunchKernelGGL(gaze_lowres_hwc_kernel, dim3(cdiv((long)B * hs * ws, 256)), dim3(256), 0, stream, img, sb, sy, sx, focus, out, B, H, W, hs,
                     ws);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int fs_grid_sample_hwc_fwd(const unsigned char* img, long sb, long sy, int sx, const float* grid, float* out, int B, int H, int W, int h, int w,
                           int nhwc_out, hipStream_t stream) {
  FS_REQUIRE(img && grid && out && B > 0 && H > 0 && W > 0 && h > 0 && w > 0 && hwc_view_ok(HwcView{img, sb, sy, sx}, B, H, W));
  hipLaunchKernelGGL(grid_sample_hwc_kernel, dim3(cdiv((long)B * h * w, 256)), dim3(256), 0, stream, img, sb, sy, sx, grid, out, B, H, W, h, w,
                     nhwc_out);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int fs_gaze_lowres_u8_fwd(const unsigned char* x, const float* focus, float* out, int B, int H, int W, int hs, int ws, hipStream_t stream) {
  FS_REQUIRE(x && focus && out && B > 0 && H > 0 && W > 0 && hs > 1 && ws > 1);
  hipLaunchKernelGGL(gaze_lowres_u8_kernel, dim3(cdiv((long)B * hs * ws, 256)), dim3(256), 0, stream, x, focus, out, B, H, W, hs, ws);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int fs_grid_sample_u8_fwd(const unsigned char* x, const float* grid, float* out, int B, int C, int H, int W, int h, int w, int nhwc_out,
                          hipStream_t stream) {
  FS_REQUIRE(x && grid && out && B > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0);
  hipLaunchKernelGGL(grid_sample_u8_kernel, dim3(cdiv((long)B * h * w, 256)), dim3(256), 0, stream, x, grid, out, B, C, H, W, h, w, nhwc_out);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // extern "C"
