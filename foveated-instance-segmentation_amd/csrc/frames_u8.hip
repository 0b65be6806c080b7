// The network's front for a frame of bytes, planar or interleaved (frame_view.h), whose pixel value is v = (float)byte / 255.0f,
// correctly rounded -- ingest_sample_kernel's expression (frontend.hip).  The network reads the frame through two gathers only, four taps
// a point each, so no fp32 frame needs to exist: the taps are converted as they are read, through the frame's reader, and everything
// after the conversion is the fp32 kernel's arithmetic, bit for bit.  An interleaved frame is read where it lies; a tap's three bytes are
// neighbours there, so a tap is one address.  The gate and the motion passes of such frames are in gaze_gate.hip and gaze_motion.hip.
//   gaze_lowres_bytes   K1 of frontend.hip on bytes (fs_gaze_lowres_u8_fwd, fs_gaze_lowres_hwc_fwd)
//   grid_sample_bytes   K5 of frontend.hip on bytes, forward only (fs_grid_sample_u8_fwd; fs_grid_sample_hwc_fwd, three channels)
// Each is written once; a kernel a layout keeps its entry point's parameters and builds its reader from them.
#include "common.h"
#include "frame_view.h"
#include "grid_taps.h"

namespace {

// gaze_lowres_kernel with the four taps converted.  Where that kernel leaves an expression to the compiler's contraction, this one spells
// the operations its code performs, so that the two stay equal bit for bit whatever the optimiser makes of the conversions around them:
// contraction is off for the whole body, whose sums and products are plain operators, and every fused multiply-add is an explicit
// __fmaf_rn.  (HIP's __fadd_rn / __fmul_rn are inline functions of plain operators compiled under -ffp-contract=fast: the pragma does
// not reach into them, and a sum of their products is still fused.)
template <class F>
__device__ __forceinline__ void gaze_lowres_bytes(const F& f, const float* __restrict__ focus, float* __restrict__ out, int B, int H, int W,
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
  // gaze_lowres_kernel leaves  ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)  to the compiler's contraction, and its
  // code (-O3, gfx950) came out differently per channel: the rows of channels 0 and 1 are r0 = fma(lx1, v01, lx0 * v00) and r1 =
  // fma(lx0, v10, lx1 * v11), channel 0 ends in fma(ly1, r1, ly0 * r0), channel 1 in fma(ly0, r0, ly1 * r1), and channel 2, whose
  // products were packed two a register, fuses nothing.  Spelled here operation for operation (profiles/r27/README.md); the test
  // against the fp32 kernel at the C ABI holds the two together.
  const auto t00 = f.px(b, y0, x0), t01 = f.px(b, y0, x1), t10 = f.px(b, y1, x0), t11 = f.px(b, y1, x1);
  float v[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[c][0] = f.tap(t00, c), v[c][1] = f.tap(t01, c);
    v[c][2] = f.tap(t10, c), v[c][3] = f.tap(t11, c);
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

__global__ __launch_bounds__(256) void gaze_lowres_u8_kernel(const unsigned char* __restrict__ x, const float* __restrict__ focus,
                                                             float* __restrict__ out, int B, int H, int W, int hs, int ws) {
  gaze_lowres_bytes(PlanarFrame<unsigned char>(x, H, W), focus, out, B, H, W, hs, ws);
}
__global__ __launch_bounds__(256) void gaze_lowres_hwc_kernel(const unsigned char* __restrict__ x, long sb, long sy, int sx,
                                                              const float* __restrict__ focus, float* __restrict__ out, int B, int H, int W,
                                                              int hs, int ws) {
  gaze_lowres_bytes(HwcFrame<0>(x, sb, sy, sx), focus, out, B, H, W, hs, ws);
}

__global__ __launch_bounds__(256) void gaze_lowres_nv12_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp, long sb,
                                                               long sy, long ub, long uy, Nv12Csc k, const float* __restrict__ focus,
                                                               float* __restrict__ out, int B, int H, int W, int hs, int ws) {
  gaze_lowres_bytes(Nv12Frame(yp, uvp, sb, sy, ub, uy, k), focus, out, B, H, W, hs, ws);
}

// C channels of image b, f the reader of that image alone -> point i of out (B,h,w,C) NHWC [nhwc_out=1] or (B,C,h,w) NCHW [nhwc_out=0],
// fp32: sample_plane's taps and chain (grid_taps.h), a tap's address formed always and read only where the tap is inside
template <class F>
__device__ __forceinline__ void grid_sample_bytes(const F& f, const float* __restrict__ grid, float* __restrict__ out, long i, int b, int C, int H,
                                                  int W, int h, int w, int nhwc_out) {
  const long pix = i - (long)b * h * w;
  const Taps t = make_taps(grid[2 * i], grid[2 * i + 1], H, W);
  const bool knw = t.oky0 & t.okx0, kne = t.oky0 & t.okx1, ksw = t.oky1 & t.okx0, kse = t.oky1 & t.okx1;
  const auto pnw = f.px(0, t.y0, t.x0), pne = f.right(pnw, 1), psw = f.down(pnw, 1), pse = f.right(psw, 1);
  for (int c = 0; c < C; ++c) {
    const float v = sample_chain(knw ? f.tap(pnw, c) : 0.f, kne ? f.tap(pne, c) : 0.f, ksw ? f.tap(psw, c) : 0.f, kse ? f.tap(pse, c) : 0.f, t);
    if (nhwc_out) out[i * C + c] = v;
    else out[((long)b * C + c) * h * w + pix] = v;
  }
}

__global__ __launch_bounds__(256) void grid_sample_u8_kernel(const unsigned char* __restrict__ x, const float* __restrict__ grid,
                                                             float* __restrict__ out, int B, int C, int H, int W, int h, int w, int nhwc_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * h * w) return;
  const int b = (int)(i / ((long)h * w));
  grid_sample_bytes(PlanarFrame<unsigned char>(x + (long)b * C * H * W, H, W), grid, out, i, b, C, H, W, h, w, nhwc_out);
}
__global__ __launch_bounds__(256) void grid_sample_hwc_kernel(const unsigned char* __restrict__ x, long sb, long sy, int sx,
                                                              const float* __restrict__ grid, float* __restrict__ out, int B, int H, int W,
                                                              int h, int w, int nhwc_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * h * w) return;
  const int b = (int)(i / ((long)h * w));
  grid_sample_bytes(HwcFrame<0>(x + (long)b * sb, sb, sy, sx), grid, out, i, b, 3, H, W, h, w, nhwc_out);
}

__global__ __launch_bounds__(256) void grid_sample_nv12_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp, long sb,
                                                               long sy, long ub, long uy, Nv12Csc k, const float* __restrict__ grid,
                                                               float* __restrict__ out, int B, int H, int W, int h, int w, int nhwc_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * h * w) return;
  const int b = (int)(i / ((long)h * w));
  grid_sample_bytes(Nv12Frame(yp + (long)b * sb, uvp + (long)b * ub, sb, sy, ub, uy, k), grid, out, i, b, 3, H, W, h, w, nhwc_out);
}

}  // namespace

extern "C" {

long fs_byte_frame_route(const unsigned char* img, long sb, long sy, int sx, int W) { return HwcFrame<0>(img, sb, sy, sx).route(W); }

int fs_gaze_lowres_hwc_fwd(const unsigned char* img, long sb, long sy, int sx, const float* focus, float* out, int B, int H, int W, int hs, int ws,
                           hipStream_t stream) {
  FS_REQUIRE(img && focus && out && B > 0 && H > 0 && W > 0 && hs > 1 && ws > 1 && HwcFrame<0>(img, sb, sy, sx).ok(B, H, W));
  hipLaunchKernelGGL(gaze_lowres_hwc_kernel, dim3(cdiv((long)B * hs * ws, 256)), dim3(256), 0, stream, img, sb, sy, sx, focus, out, B, H, W, hs,
                     ws);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int fs_grid_sample_hwc_fwd(const unsigned char* img, long sb, long sy, int sx, const float* grid, float* out, int B, int H, int W, int h, int w,
                           int nhwc_out, hipStream_t stream) {
  FS_REQUIRE(img && grid && out && B > 0 && H > 0 && W > 0 && h > 0 && w > 0 && HwcFrame<0>(img, sb, sy, sx).ok(B, H, W));
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

int fs_gaze_lowres_nv12_fwd(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu,
                            int gv, int bu, const float* focus, float* out, int B, int H, int W, int hs, int ws, hipStream_t stream) {
  const Nv12Frame f(yp, uvp, sb, sy, ub, uy, Nv12Csc{yo, yg, rv, gu, gv, bu});
  FS_REQUIRE(f && focus && out && B > 0 && H > 0 && W > 0 && hs > 1 && ws > 1 && f.ok(B, H, W));
  hipLaunchKernelGGL(gaze_lowres_nv12_kernel, dim3(cdiv((long)B * hs * ws, 256)), dim3(256), 0, stream, yp, uvp, sb, sy, ub, uy, f.k, focus, out, B,
                     H, W, hs, ws);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int fs_grid_sample_nv12_fwd(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu,
                            int gv, int bu, const float* grid, float* out, int B, int H, int W, int h, int w, int nhwc_out, hipStream_t stream) {
  const Nv12Frame f(yp, uvp, sb, sy, ub, uy, Nv12Csc{yo, yg, rv, gu, gv, bu});
  FS_REQUIRE(f && grid && out && B > 0 && H > 0 && W > 0 && h > 0 && w > 0 && f.ok(B, H, W));
  hipLaunchKernelGGL(grid_sample_nv12_kernel, dim3(cdiv((long)B * h * w, 256)), dim3(256), 0, stream, yp, uvp, sb, sy, ub, uy, f.k, grid, out, B, H,
                     W, h, w, nhwc_out);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // extern "C"
