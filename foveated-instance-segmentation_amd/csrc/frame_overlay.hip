// Showing the record: the gazed instance drawn onto the frame it was found in (no counterpart on the device in the reference, which draws
// with matplotlib and PIL on the host -- eval.py:70-83 visualize_result, utils.py:207-221 colorEncode --: UNPINNED, a definition of this
// library's; include/fovealseg.h "showing the record" states the rule).  All of it is integer work on pixel codes:
//   overlay   one launch: every pixel of every viewer reads its three codes through the frame's reader (frame_view.h), its bit of the
//             record's mask and of the outline band, applies the first of marker / box / outline / tint / dim that holds and stores three
//             or four bytes through the frame's writer.  Every output byte is stored once, plainly: no atomics, nothing to zero.
//   encode    the class map of predict() as colours: palette[label], black for a label outside the palette; the same writer.
// A source whose sixteen-pixel pieces are aligned on both sides takes the vector form: a lane owns sixteen pixels of a row -- the
// reader's load16 gives them in planar order in registers (twelve 16-byte loads of an fp32 frame, coded as they arrive), a half word
// of bits and of band decides them, and the writer stores sixteen bytes a channel, or re-interleaves them (v_perm_b32: hwc_join3 /
// hwc_join4) into three or four 16-byte pieces that leave through LDS so that neighbouring lanes store neighbouring bytes.
// Everything else -- odd widths, pitches and pointers -- takes the one-pixel form over the same reader and writer.  A workgroup reads
// its pixels before it stores them and owns them alone, so out may be img where the two descriptions are the same.
#include "mask_words.h"
#include "frame_view.h"

namespace {

constexpr int OVL_THREADS = 256;
constexpr int OVL_STYLE = 20;                          // ints a style row
constexpr int OVL_FAR = 65536;                         // box edges are clamped to +-OVL_FAR: beyond every x - t and x + t

// what follows the frame in the arguments of the three entry points
struct OverlayArgs {
  const unsigned int* bits;
  const unsigned int* band;
  const long long* stats;
  const float* focus;
  const long long* live;
  long live_stride;
  const int* style;
  int S;
};

// a viewer's rule, from its style row, record and gaze: what every pixel of the viewer compares with
struct OverlayRule {
  int ta[3], keep, dim;                                // tint_c * a, 256 - a
  int line[3], box[3], mark[3];
  int r, r2, in2, py, px;                              // marker: r = 0 switches it off
  int t, bx0, bx1, by0, by1;                           // box: t = 0 switches it off; [bx0, bx1) x [by0, by1) clamped to +-OVL_FAR
  bool live, outline;
};

__device__ __forceinline__ int ovl_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int ovl_far(long long v) { return v < -OVL_FAR ? -OVL_FAR : (v > OVL_FAR ? OVL_FAR : (int)v); }

// No style value and no stats value forms an address: every entry is clamped, and the box is compared only.  lo + len is taken without
// overflow (len > 0): lo < 0 cannot overflow, lo >= 0 saturates; the clamp to +-OVL_FAR keeps every comparison with x - t and x + t.
__device__ __forceinline__ OverlayRule overlay_rule(const OverlayArgs& A, size_t b, int H, int W) {
  OverlayRule R;
  const int* st = A.style + (A.S == 1 ? 0 : b) * OVL_STYLE;
  const int a = ovl_clamp(st[3], 256);
  R.keep = 256 - a;
  R.dim = ovl_clamp(st[7], 256);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    R.ta[c] = ovl_clamp(st[c], 255) * a;
    R.line[c] = ovl_clamp(st[4 + c], 255);
    R.box[c] = ovl_clamp(st[8 + c], 255);
    R.mark[c] = ovl_clamp(st[12 + c], 255);
  }
  R.live = A.live == nullptr || A.live[b * (size_t)A.live_stride] != 0;
  R.outline = R.live && A.band != nullptr && st[17] != 0;
  R.r = 0, R.r2 = 0, R.in2 = 0, R.py = 0, R.px = 0;
  if (A.focus != nullptr) {
    const int r = ovl_clamp(st[15], MASK_MAX_SIDE), w = ovl_clamp(st[16], MASK_MAX_SIDE);     // squared distances stay below 2^30: ints
    const int in = r > w ? r - w : 0;
    R.r = r, R.r2 = r * r, R.in2 = in * in;
    R.py = mask_gaze_px(mask_gaze16(A.focus[2 * b], H)), R.px = mask_gaze_px(mask_gaze16(A.focus[2 * b + 1], W));
  }
  R.t = 0, R.bx0 = 0, R.bx1 = 0, R.by0 = 0, R.by1 = 0;
  if (A.stats != nullptr && R.live) {
    const long long x0 = A.stats[b * 6 + 1], y0 = A.stats[b * 6 + 2], bw = A.stats[b * 6 + 3], bh = A.stats[b * 6 + 4];
    if (bw > 0 && bh > 0) {
      const long long top = 0x7fffffffffffffffLL;
      const long long x1 = (x0 > 0 && bw > top - x0) ? top : x0 + bw, y1 = (y0 > 0 && bh > top - y0) ? top : y0 + bh;
      R.t = ovl_clamp(st[11], MASK_MAX_SIDE);
      R.bx0 = ovl_far(x0), R.bx1 = ovl_far(x1), R.by0 = ovl_far(y0), R.by1 = ovl_far(y1);
    }
  }
  return R;
}

// what a row settles for its pixels
struct OverlayRow {
  int dy2;
  bool mark, box, edge;
};
__device__ __forceinline__ OverlayRow overlay_row(const OverlayRule& R, int y) {
  OverlayRow r;
  const int dy = y - R.py;
  r.dy2 = dy * dy;
  r.mark = R.r > 0 && r.dy2 <= R.r2;
  r.box = R.t > 0 && y >= R.by0 && y < R.by1;
  r.edge = R.by0 > y - R.t || R.by1 <= y + R.t;
  return r;
}

// the first of marker, box, outline, tint, dim that holds for pixel (y, x) with the codes s
__device__ __forceinline__ void overlay_pixel(const OverlayRule& R, const OverlayRow& row, int x, bool bit, bool bnd, const int* s, int* o) {
  const int m = bit ? R.keep : R.dim;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (s[c] * m + (bit ? R.ta[c] : 0) + 128) >> 8;
  if (bnd) o[0] = R.line[0], o[1] = R.line[1], o[2] = R.line[2];
  if (row.box && x >= R.bx0 && x < R.bx1 && (row.edge || R.bx0 > x - R.t || R.bx1 <= x + R.t)) o[0] = R.box[0], o[1] = R.box[1], o[2] = R.box[2];
  if (row.mark) {
    const int dx = x - R.px, d2 = row.dy2 + dx * dx;
    if (d2 <= R.r2 && d2 >= R.in2) o[0] = R.mark[0], o[1] = R.mark[1], o[2] = R.mark[2];
  }
}

// The one-pixel form, for any source, destination, width and alignment: bpi workgroups a viewer, a lane a pixel.
template <class F>
__device__ __forceinline__ void overlay_px(const F& f, const OverlayArgs& A, const FrameWriter<0>& o, int H, int W, unsigned int bpi) {
  const size_t b = blockIdx.x / bpi;
  const unsigned int i = (blockIdx.x - (unsigned int)b * bpi) * OVL_THREADS + threadIdx.x;
  if (i >= (unsigned int)(H * W)) return;
  const int y = (int)(i / (unsigned int)W), x = (int)(i - (unsigned int)y * W);
  const OverlayRule R = overlay_rule(A, b, H, W);
  const OverlayRow row = overlay_row(R, y);
  const size_t word = (b * H + y) * (size_t)mask_row_words(W) + (x >> 5);
  const bool bit = R.live && mask_bit(A.bits[word], x) != 0;
  const bool bnd = R.outline && mask_bit(A.band[word], x) != 0;
  const auto a = f.px(b, y, x);
  const int s[3] = {f.code(a, 0), f.code(a, 1), f.code(a, 2)};
  int c[3];
  overlay_pixel(R, row, x, bit, bnd, s, c);
  o.store1(b, y, x, c[0], c[1], c[2]);
}

// Sixteen pixels of a row in planar order in registers, v[c] = sixteen codes of channel c: the reader's load16 of a byte frame; twelve
// 16-byte loads of an fp32 frame, each value's code taken as it arrives.
template <class F>
__device__ __forceinline__ void overlay_load16(const F& f, const unsigned char* a, u32x4* v) { f.load16(a, v); }
__device__ __forceinline__ void overlay_load16(const Nv12Frame& f, const Nv12Px& a, u32x4* v) { f.load16(a, v); }
__device__ __forceinline__ void overlay_load16(const PlanarFrame<float>& f, const float* a, u32x4* v) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f32x4 t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = *reinterpret_cast<const f32x4*>(a + c * f.plane + 4 * q);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      v[c][q] = (unsigned int)pixel_q(t[q].x) | ((unsigned int)pixel_q(t[q].y) << 8) | ((unsigned int)pixel_q(t[q].z) << 16) | ((unsigned int)pixel_q(t[q].w) << 24);
  }
}

// An interleaved destination's sixteen-pixel pieces leave through LDS: a lane's 48 or 64 bytes lie 48 or 64 bytes from its neighbour's, so
// stored by their own lanes a store instruction of a wave touches a quarter or a third of every line it reaches (profiles/r34/README.md:
// u8 -> RGBA 120 us against 85 us into planes).  The workgroup lays its pieces down in memory order, and lane j then stores the 16-byte
// pieces j, j + 256, ...: neighbours store neighbouring bytes.  e0 = the workgroup's first unit; every lane of the workgroup calls.
template <int OX>
__device__ __forceinline__ void overlay_store_staged(const FrameWriter<OX>& o, size_t b, unsigned int e0, unsigned int units, unsigned int w16,
                                                     const unsigned int (*v)[4]) {
  __shared__ u32x4 stage[OVL_THREADS * OX];
  u32x4 m[OX];
  o.join16(v, m);
#pragma unroll
  for (int k = 0; k < OX; ++k) stage[threadIdx.x * OX + k] = m[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < OX; ++k) {
    const unsigned int c = k * OVL_THREADS + threadIdx.x, lane = c / OX, part = c - lane * OX, e = e0 + lane;
    if (e < units) {
      const int y = (int)(e / w16), x = (int)(e - (unsigned int)y * w16) * 16;
      *reinterpret_cast<u32x4*>(o.piece(b, y, x) + part * 16) = stage[c];
    }
  }
}

// The sixteen-pixel form (the reader's and the writer's wide): bpi workgroups a viewer, a lane sixteen pixels of a row.  Every read of a
// workgroup's pixels comes before its stores (a lane's own before its own for a planar destination, the barrier of the staged store for
// an interleaved one), and workgroups own disjoint pixels: out may be img.
template <class F, int OX>
__device__ __forceinline__ void overlay_wide(const F& f, const OverlayArgs& A, const FrameWriter<OX>& o, int H, int W, unsigned int bpi) {
  const size_t b = blockIdx.x / bpi;
  const unsigned int e0 = (blockIdx.x - (unsigned int)b * bpi) * OVL_THREADS, e = e0 + threadIdx.x;
  const unsigned int w16 = (unsigned int)W >> 4, units = (unsigned int)H * w16;
  const bool mine = e < units;
  const int y = mine ? (int)(e / w16) : 0, x = mine ? (int)(e - (unsigned int)y * w16) * 16 : 0;
  unsigned int out[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
  if (mine) {
    const OverlayRule R = overlay_rule(A, b, H, W);
    const OverlayRow row = overlay_row(R, y);
    const size_t word = (b * H + y) * (size_t)mask_row_words(W) + (x >> 5);
    const unsigned int bits = R.live ? (A.bits[word] >> (x & 16)) & 0xffffu : 0u;
    const unsigned int band = R.outline ? (A.band[word] >> (x & 16)) & 0xffffu : 0u;
    u32x4 v[3];
    overlay_load16(f, f.px(b, y, x), v);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned int w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * q + j;
        const int s[3] = {(int)((v[0][q] >> (8 * j)) & 255u), (int)((v[1][q] >> (8 * j)) & 255u), (int)((v[2][q] >> (8 * j)) & 255u)};
        int c[3];
        overlay_pixel(R, row, x + k, ((bits >> k) & 1u) != 0, ((band >> k) & 1u) != 0, s, c);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) w[ch] |= (unsigned int)c[ch] << (8 * j);
      }
      out[0][q] = w[0], out[1][q] = w[1], out[2][q] = w[2];
    }
  }
  if (OX == 1) {
    if (mine) o.store16(b, y, x, out);
  } else {
    overlay_store_staged(o, b, e0, units, w16, out);
  }
}

// The kernels: each source layout keeps the parameters of its entry point, raw pointers and scalars, and builds its reader and writer
// from them.  img and out carry no __restrict__: they may be one buffer.
__global__ __launch_bounds__(OVL_THREADS) void overlay_kernel(const float* img, OverlayArgs A, unsigned char* out, long ob, long oy, int ox,
                                                              int H, int W, unsigned int bpi) {
  overlay_px(PlanarFrame<float>(img, H, W), A, FrameWriter<0>(out, ob, oy, ox, H, W), H, W, bpi);
}
__global__ __launch_bounds__(OVL_THREADS) void overlay_u8_kernel(const unsigned char* img, OverlayArgs A, unsigned char* out, long ob, long oy,
                                                                 int ox, int H, int W, unsigned int bpi) {
  overlay_px(PlanarFrame<unsigned char>(img, H, W), A, FrameWriter<0>(out, ob, oy, ox, H, W), H, W, bpi);
}
__global__ __launch_bounds__(OVL_THREADS) void overlay_hwc_kernel(const unsigned char* img, long sb, long sy, int sx, OverlayArgs A,
                                                                  unsigned char* out, long ob, long oy, int ox, int H, int W, unsigned int bpi) {
  overlay_px(HwcFrame<0>(img, sb, sy, sx), A, FrameWriter<0>(out, ob, oy, ox, H, W), H, W, bpi);
}
template <int OX>
__global__ __launch_bounds__(OVL_THREADS) void overlay_f32_wide_kernel(const float* img, OverlayArgs A, unsigned char* out, long ob, long oy, int H,
                                                                       int W, unsigned int bpi) {
  overlay_wide(PlanarFrame<float>(img, H, W), A, FrameWriter<OX>(out, ob, oy, OX, H, W), H, W, bpi);
}
template <int OX>
__global__ __launch_bounds__(OVL_THREADS) void overlay_u8_wide_kernel(const unsigned char* img, OverlayArgs A, unsigned char* out, long ob, long oy,
                                                                      int H, int W, unsigned int bpi) {
  overlay_wide(PlanarFrame<unsigned char>(img, H, W), A, FrameWriter<OX>(out, ob, oy, OX, H, W), H, W, bpi);
}
template <int SX, int OX>
__global__ __launch_bounds__(OVL_THREADS) void overlay_hwc_wide_kernel(const unsigned char* img, long sb, long sy, OverlayArgs A,
                                                                       unsigned char* out, long ob, long oy, int H, int W, unsigned int bpi) {
  overlay_wide(HwcFrame<SX>(img, sb, sy, SX), A, FrameWriter<OX>(out, ob, oy, OX, H, W), H, W, bpi);
}

__global__ __launch_bounds__(OVL_THREADS) void overlay_nv12_kernel(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy,
                                                                   Nv12Csc k, OverlayArgs A, unsigned char* out, long ob, long oy, int ox, int H,
                                                                   int W, unsigned int bpi) {
  overlay_px(Nv12Frame(yp, uvp, sb, sy, ub, uy, k), A, FrameWriter<0>(out, ob, oy, ox, H, W), H, W, bpi);
}
template <int OX>
__global__ __launch_bounds__(OVL_THREADS) void overlay_nv12_wide_kernel(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub,
                                                                        long uy, Nv12Csc k, OverlayArgs A, unsigned char* out, long ob, long oy,
                                                                        int H, int W, unsigned int bpi) {
  overlay_wide(Nv12Frame(yp, uvp, sb, sy, ub, uy, k), A, FrameWriter<OX>(out, ob, oy, OX, H, W), H, W, bpi);
}

// is out the frame's own memory?  (an NV12 frame is never what the pass writes: out at either of its planes is refused, since no
// destination has its description)
template <class F>
bool overlay_in_place(const F& f, const unsigned char* out) { return (const void*)f.p == (const void*)out; }
bool overlay_in_place(const Nv12Frame& f, const unsigned char* out) { return out == f.yp || out == f.uvp; }
bool overlay_same(const Nv12Frame&, const FrameWriter<0>&, int, int, int) { return false; }

// out may be img only where the two descriptions are the same (an image step counts where there is more than one image)
bool overlay_same(const PlanarFrame<float>&, const FrameWriter<0>&, int, int, int) { return false; }
bool overlay_same(const PlanarFrame<unsigned char>&, const FrameWriter<0>& o, int B, int H, int W) {
  return o.ox == 1 && (B == 1 || o.ob == 3 * (long)H * W);
}
bool overlay_same(const HwcFrame<0>& f, const FrameWriter<0>& o, int B, int, int) { return o.ox == f.sx && o.oy == f.sy && (B == 1 || o.ob == f.sb); }

// the launch by the source's layout; wide = the sixteen-pixel form
void overlay_launch(const PlanarFrame<float>& f, const FrameWriter<0>& o, bool wide, dim3 grid, hipStream_t stream, const OverlayArgs& A, int H, int W,
                    unsigned int bpi) {
  const dim3 block(OVL_THREADS);
  if (!wide) hipLaunchKernelGGL(overlay_kernel, grid, block, 0, stream, f.p, A, o.p, o.ob, o.oy, o.ox, H, W, bpi);
  else if (o.ox == 1) hipLaunchKernelGGL(overlay_f32_wide_kernel<1>, grid, block, 0, stream, f.p, A, o.p, o.ob, o.oy, H, W, bpi);
  else if (o.ox == 3) hipLaunchKernelGGL(overlay_f32_wide_kernel<3>, grid, block, 0, stream, f.p, A, o.p, o.ob, o.oy, H, W, bpi);
  else hipLaunchKernelGGL(overlay_f32_wide_kernel<4>, grid, block, 0, stream, f.p, A, o.p, o.ob, o.oy, H, W, bpi);
}
void overlay_launch(const PlanarFrame<unsigned char>& f, const FrameWriter<0>& o, bool wide, dim3 grid, hipStream_t stream, const OverlayArgs& A,
                    int H, int W, unsigned int bpi) {
  const dim3 block(OVL_THREADS);
  if (!wide) hipLaunchKernelGGL(overlay_u8_kernel, grid, block, 0, stream, f.p, A, o.p, o.ob, o.oy, o.ox, H, W, bpi);
  else if (o.ox == 1) hipLaunchKernelGGL(overlay_u8_wide_kernel<1>, grid, block, 0, stream, f.p, A, o.p, o.ob, o.oy, H, W, bpi);
  else if (o.ox == 3) hipLaunchKernelGGL(overlay_u8_wide_kernel<3>, grid, block, 0, stream, f.p, A, o.p, o.ob, o.oy, H, W, bpi);
  else hipLaunchKernelGGL(overlay_u8_wide_kernel<4>, grid, block, 0, stream, f.p, A, o.p, o.ob, o.oy, H, W, bpi);
}
template <int SX>
void overlay_launch_hwc_wide(const HwcFrame<0>& f, const FrameWriter<0>& o, dim3 grid, hipStream_t stream, const OverlayArgs& A, int H, int W,
                             unsigned int bpi) {
  const dim3 block(OVL_THREADS);
  if (o.ox == 1) hipLaunchKernelGGL((overlay_hwc_wide_kernel<SX, 1>), grid, block, 0, stream, f.p, f.sb, f.sy, A, o.p, o.ob, o.oy, H, W, bpi);
  else if (o.ox == 3) hipLaunchKernelGGL((overlay_hwc_wide_kernel<SX, 3>), grid, block, 0, stream, f.p, f.sb, f.sy, A, o.p, o.ob, o.oy, H, W, bpi);
  else hipLaunchKernelGGL((overlay_hwc_wide_kernel<SX, 4>), grid, block, 0, stream, f.p, f.sb, f.sy, A, o.p, o.ob, o.oy, H, W, bpi);
}
void overlay_launch(const HwcFrame<0>& f, const FrameWriter<0>& o, bool wide, dim3 grid, hipStream_t stream, const OverlayArgs& A, int H, int W,
                    unsigned int bpi) {
  if (!wide) hipLaunchKernelGGL(overlay_hwc_kernel, grid, dim3(OVL_THREADS), 0, stream, f.p, f.sb, f.sy, f.sx, A, o.p, o.ob, o.oy, o.ox, H, W, bpi);
  else if (f.sx == 3) overlay_launch_hwc_wide<3>(f, o, grid, stream, A, H, W, bpi);
  else overlay_launch_hwc_wide<4>(f, o, grid, stream, A, H, W, bpi);
}

void overlay_launch(const Nv12Frame& f, const FrameWriter<0>& o, bool wide, dim3 grid, hipStream_t stream, const OverlayArgs& A, int H, int W,
                    unsigned int bpi) {
  const dim3 block(OVL_THREADS);
  if (!wide)
    hipLaunchKernelGGL(overlay_nv12_kernel, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, A, o.p, o.ob, o.oy, o.ox, H, W, bpi);
  else if (o.ox == 1)
    hipLaunchKernelGGL(overlay_nv12_wide_kernel<1>, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, A, o.p, o.ob, o.oy, H, W, bpi);
  else if (o.ox == 3)
    hipLaunchKernelGGL(overlay_nv12_wide_kernel<3>, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, A, o.p, o.ob, o.oy, H, W, bpi);
  else
    hipLaunchKernelGGL(overlay_nv12_wide_kernel<4>, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, A, o.p, o.ob, o.oy, H, W, bpi);
}

bool overlay_sizes_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && H <= MASK_MAX_SIDE && W <= MASK_MAX_SIDE && (long)H * W < MASK_INT_LIMIT;
}

// fs_frame_overlay / _u8 / _hwc: the checks and the choice of the form, here alone
template <class F>
int overlay_run(const F& f, const OverlayArgs& A, unsigned char* out, long ob, long oy, int ox, int B, int H, int W, hipStream_t stream) {
  const FrameWriter<0> o(out, ob, oy, ox, H, W);
  FS_REQUIRE(f && A.bits && A.style && out && overlay_sizes_ok(B, H, W) && (A.S == 1 || A.S == B));
  FS_REQUIRE(f.ok(B, H, W) && o.ok(B, H, W) && (A.live == nullptr || A.live_stride >= 1));
  FS_REQUIRE(!overlay_in_place(f, out) || overlay_same(f, o, B, H, W));
  const bool wide = f.wide(W) && o.wide(W);             // the writer's W % 16 == 0 goes for an fp32 frame too, whose own rule is W % 4
  const long bpi = ((long)H * (wide ? W / 16 : W) + OVL_THREADS - 1) / OVL_THREADS;
  FS_REQUIRE((long)B * bpi < MASK_INT_LIMIT);
  overlay_launch(f, o, wide, dim3((unsigned)((long)B * bpi)), stream, A, H, W, (unsigned int)bpi);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// out <- palette[label], (0, 0, 0) for a label outside 0 .. K-1: the label forms an address only inside the palette.  SIXTEEN: a lane
// takes sixteen labels of a row (eight 16-byte loads) and stores through the writer's sixteen-pixel form; one label a lane otherwise.
__device__ __forceinline__ void encode_label(long long l, const unsigned char* __restrict__ palette, int K, int* c) {
  const bool in = l >= 0 && l < (long long)K;
  const unsigned char* p = palette + (in ? (size_t)l * 3 : 0);
  c[0] = in ? (int)p[0] : 0, c[1] = in ? (int)p[1] : 0, c[2] = in ? (int)p[2] : 0;
}
template <int OX>
__global__ __launch_bounds__(OVL_THREADS) void color_encode_kernel(const long long* __restrict__ labels, const unsigned char* __restrict__ palette,
                                                                   int K, unsigned char* __restrict__ out, long ob, long oy, int ox, int H, int W,
                                                                   unsigned int bpi) {
  const FrameWriter<OX> o(out, ob, oy, OX > 0 ? OX : ox, H, W);
  const size_t b = blockIdx.x / bpi;
  const unsigned int e = (blockIdx.x - (unsigned int)b * bpi) * OVL_THREADS + threadIdx.x;
  const long long* lb = labels + b * (size_t)H * W;
  if (OX == 0) {
    if (e >= (unsigned int)(H * W)) return;
    const int y = (int)(e / (unsigned int)W), x = (int)(e - (unsigned int)y * W);
    int c[3];
    encode_label(lb[e], palette, K, c);
    o.store1(b, y, x, c[0], c[1], c[2]);
  } else {
    const unsigned int w16 = (unsigned int)W >> 4;
    if (e >= (unsigned int)H * w16) return;
    const int y = (int)(e / w16), x = (int)(e - (unsigned int)y * w16) * 16;
    const u32x4* src = reinterpret_cast<const u32x4*>(lb + (size_t)y * W + x);
    unsigned int v[3][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned int w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; j += 2) {
        const u32x4 two = src[(4 * q + j) >> 1];
        const long long l0 = (long long)(((unsigned long long)two.y << 32) | two.x), l1 = (long long)(((unsigned long long)two.w << 32) | two.z);
        int c0[3], c1[3];
        encode_label(l0, palette, K, c0);
        encode_label(l1, palette, K, c1);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) w[ch] |= ((unsigned int)c0[ch] << (8 * j)) | ((unsigned int)c1[ch] << (8 * j + 8));
      }
      v[0][q] = w[0], v[1][q] = w[1], v[2][q] = w[2];
    }
    o.store16(b, y, x, v);
  }
}

}  // namespace

extern "C" {

int fs_frame_overlay(const float* img, const unsigned int* bits, const unsigned int* band, const long long* stats, const float* focus,
                     const long long* live, long live_stride, const int* style, int S, unsigned char* out, long ob, long oy, int ox, int B, int H,
                     int W, hipStream_t stream) {
  const OverlayArgs A = {bits, band, stats, focus, live, live_stride, style, S};
  return overlay_run(PlanarFrame<float>(img, H, W), A, out, ob, oy, ox, B, H, W, stream);
}

int fs_frame_overlay_u8(const unsigned char* img, const unsigned int* bits, const unsigned int* band, const long long* stats, const float* focus,
                        const long long* live, long live_stride, const int* style, int S, unsigned char* out, long ob, long oy, int ox, int B,
                        int H, int W, hipStream_t stream) {
  const OverlayArgs A = {bits, band, stats, focus, live, live_stride, style, S};
  return overlay_run(PlanarFrame<unsigned char>(img, H, W), A, out, ob, oy, ox, B, H, W, stream);
}

int fs_frame_overlay_hwc(const unsigned char* img, long sb, long sy, int sx, const unsigned int* bits, const unsigned int* band,
                         const long long* stats, const float* focus, const long long* live, long live_stride, const int* style, int S,
                         unsigned char* out, long ob, long oy, int ox, int B, int H, int W, hipStream_t stream) {
  const OverlayArgs A = {bits, band, stats, focus, live, live_stride, style, S};
  return overlay_run(HwcFrame<0>(img, sb, sy, sx), A, out, ob, oy, ox, B, H, W, stream);
}

int fs_frame_overlay_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu,
                          int gv, int bu, const unsigned int* bits, const unsigned int* band, const long long* stats, const float* focus,
                          const long long* live, long live_stride, const int* style, int S, unsigned char* out, long ob, long oy, int ox, int B,
                          int H, int W, hipStream_t stream) {
  const OverlayArgs A = {bits, band, stats, focus, live, live_stride, style, S};
  return overlay_run(Nv12Frame(yp, uvp, sb, sy, ub, uy, Nv12Csc{yo, yg, rv, gu, gv, bu}), A, out, ob, oy, ox, B, H, W, stream);
}

int fs_color_encode(const long long* labels, const unsigned char* palette, unsigned char* out, long ob, long oy, int ox, int B, int H, int W,
                    int K, hipStream_t stream) {
  const FrameWriter<0> o(out, ob, oy, ox, H, W);
  FS_REQUIRE(labels && palette && out && K >= 1 && overlay_sizes_ok(B, H, W) && o.ok(B, H, W));
  const bool wide = o.wide(W) && ((uintptr_t)labels & 15) == 0;
  const long bpi = ((long)H * (wide ? W / 16 : W) + OVL_THREADS - 1) / OVL_THREADS;
  FS_REQUIRE((long)B * bpi < MASK_INT_LIMIT);
  const dim3 grid((unsigned)((long)B * bpi)), block(OVL_THREADS);
  if (!wide) hipLaunchKernelGGL(color_encode_kernel<0>, grid, block, 0, stream, labels, palette, K, out, ob, oy, ox, H, W, (unsigned int)bpi);
  else if (ox == 1) hipLaunchKernelGGL(color_encode_kernel<1>, grid, block, 0, stream, labels, palette, K, out, ob, oy, ox, H, W, (unsigned int)bpi);
  else if (ox == 3) hipLaunchKernelGGL(color_encode_kernel<3>, grid, block, 0, stream, labels, palette, K, out, ob, oy, ox, H, W, (unsigned int)bpi);
  else hipLaunchKernelGGL(color_encode_kernel<4>, grid, block, 0, stream, labels, palette, K, out, ob, oy, ox, H, W, (unsigned int)bpi);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // extern "C"
