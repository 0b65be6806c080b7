// An NV12 frame as RGB bytes (frame_view.h: Nv12Frame; include/fovealseg.h "frames as NV12"; no counterpart in the reference, which reads
// image files: UNPINNED).  Every pass of the serving side reads an NV12 frame where it lies (fs_*_nv12), so nobody
// needs this conversion in front of them; it is the frame a caller displays, and the planar twin the tests hold those passes to.  All of
// it is integer work: 1.5 bytes a pixel read, 3 or 4 written.
//   nv12_rgb_wide   sixteen pixels a lane: the reader's load16 -- one 16-byte load of luma, one of chroma -- into the writer's store16
//                   (the reader's and the writer's wide: W % 16 == 0, both sides 16-byte aligned)
//   nv12_rgb_px     one pixel a lane, for any width, pitch and alignment
#include "common.h"
#include "frame_view.h"

namespace {

constexpr int NV12_THREADS = 256;
constexpr long NV12_INT_LIMIT = 2147483647L;

template <int OX>
__global__ __launch_bounds__(NV12_THREADS) void nv12_rgb_wide_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp,
                                                                     long sb, long sy, long ub, long uy, Nv12Csc k, unsigned char* __restrict__ out,
                                                                     long ob, long oy, int H, int W, unsigned int bpi) {
  const Nv12Frame f(yp, uvp, sb, sy, ub, uy, k);
  const FrameWriter<OX> o(out, ob, oy, OX, H, W);
  const size_t b = blockIdx.x / bpi;
  const unsigned int e = (blockIdx.x - (unsigned int)b * bpi) * NV12_THREADS + threadIdx.x;
  const unsigned int w16 = (unsigned int)W >> 4;
  if (e >= (unsigned int)H * w16) return;
  const int y = (int)(e / w16), x = (int)(e - (unsigned int)y * w16) * 16;
  u32x4 v[3];
  f.load16(f.px(b, y, x), v);
  const unsigned int m[3][4] = {{v[0].x, v[0].y, v[0].z, v[0].w}, {v[1].x, v[1].y, v[1].z, v[1].w}, {v[2].x, v[2].y, v[2].z, v[2].w}};
  o.store16(b, y, x, m);
}

__global__ __launch_bounds__(NV12_THREADS) void nv12_rgb_px_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp, long sb,
                                                                   long sy, long ub, long uy, Nv12Csc k, unsigned char* __restrict__ out, long ob,
                                                                   long oy, int ox, int H, int W, unsigned int bpi) {
  const Nv12Frame f(yp, uvp, sb, sy, ub, uy, k);
  const FrameWriter<0> o(out, ob, oy, ox, H, W);
  const size_t b = blockIdx.x / bpi;
  const unsigned int i = (blockIdx.x - (unsigned int)b * bpi) * NV12_THREADS + threadIdx.x;
  if (i >= (unsigned int)(H * W)) return;
  const int y = (int)(i / (unsigned int)W), x = (int)(i - (unsigned int)y * W);
  const Nv12Px a = f.px(b, y, x);
  o.store1(b, y, x, f.code(a, 0), f.code(a, 1), f.code(a, 2));
}

}  // namespace

extern "C" {

long fs_nv12_frame_route(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int W) {
  return Nv12Frame(yp, uvp, sb, sy, ub, uy, Nv12Csc{0, 256, 0, 0, 0, 0}).route(W);
}

int fs_nv12_to_rgb(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu, int gv,
                   int bu, unsigned char* out, long ob, long oy, int ox, int B, int H, int W, hipStream_t stream) {
  const Nv12Frame f(yp, uvp, sb, sy, ub, uy, Nv12Csc{yo, yg, rv, gu, gv, bu});
  const FrameWriter<0> o(out, ob, oy, ox, H, W);
  FS_REQUIRE(f && out && B > 0 && H > 0 && W > 0 && (long)H * W < NV12_INT_LIMIT && f.ok(B, H, W) && o.ok(B, H, W));
  FS_REQUIRE(out != yp && out != uvp);                  // no destination has the frame's description: never in place
  const bool wide = f.wide(W) && o.wide(W);
  const long bpi = ((long)H * (wide ? W / 16 : W) + NV12_THREADS - 1) / NV12_THREADS;
  FS_REQUIRE((long)B * bpi < NV12_INT_LIMIT);
  const dim3 grid((unsigned)((long)B * bpi)), block(NV12_THREADS);
  if (!wide)
    hipLaunchKernelGGL(nv12_rgb_px_kernel, grid, block, 0, stream, yp, uvp, sb, sy, ub, uy, f.k, out, ob, oy, ox, H, W, (unsigned int)bpi);
  else if (ox == 1)
    hipLaunchKernelGGL(nv12_rgb_wide_kernel<1>, grid, block, 0, stream, yp, uvp, sb, sy, ub, uy, f.k, out, ob, oy, H, W, (unsigned int)bpi);
  else if (ox == 3)
    hipLaunchKernelGGL(nv12_rgb_wide_kernel<3>, grid, block, 0, stream, yp, uvp, sb, sy, ub, uy, f.k, out, ob, oy, H, W, (unsigned int)bpi);
  else
    hipLaunchKernelGGL(nv12_rgb_wide_kernel<4>, grid, block, 0, stream, yp, uvp, sb, sy, ub, uy, f.k, out, ob, oy, H, W, (unsigned int)bpi);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // extern "C"
